"""CPU: the ctypes binding that hs_pose_amd._lib derives from include/hsp.h, held to the host C++ compiler's own view of the same
header -- every prototype's return and parameter types, every struct's size, field offsets and field types, every constant's value --
and the header reader's refusals: whatever it does not understand is an error that quotes the declaration, never a skipped one.

The names fed to the generated program are the reader's output; the types, layouts and values it prints are the compiler's.  A name
the reader dropped is caught by tests/test_abi_host.py (an independent regex over the header) and by the counts below."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from hs_pose_amd import _lib

PROGRAM = r"""
#include "hsp.h"
#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>
template <class T> std::string code() {
    if (std::is_same<T, const char *>::value) return "s";
    if (std::is_pointer<T>::value) return "p";
    if (std::is_floating_point<T>::value) return "f" + std::to_string(sizeof(T));
    if (std::is_integral<T>::value) return (std::is_signed<T>::value ? "i" : "u") + std::to_string(sizeof(T));
    return "?";                         /* a struct by value, void, anything else: matches nothing the binding may hold */
}
template <class F> struct Fn;            /* instantiated on decltype(&fn): unevaluated, so nothing has to link */
template <class R, class... A> struct Fn<R (*)(A...)> {
    static void print(const char *name) {
        std::string s = std::string("F ") + name + " " + code<R>();
        int unused[] = {0, (s += " " + code<A>(), 0)...};
        (void)unused;
        std::puts(s.c_str());
    }
};
#define FIELD(T, f) std::printf(" %s:%zu:%zu:%s", #f, offsetof(T, f), sizeof(((T *)0)->f), code<decltype(T::f)>().c_str())
int main() {
@BODY@
    return 0;
}
"""


def _code(ct):
    """the generated program's code for a ctypes type"""
    if ct in (ctypes.c_void_p, ctypes.c_char_p):
        return "p" if ct is ctypes.c_void_p else "s"
    if ct in (ctypes.c_float, ctypes.c_double):
        return f"f{ctypes.sizeof(ct)}"
    return ("i" if ct(-1).value < 0 else "u") + str(ctypes.sizeof(ct))


def _header_text():
    with open(_lib.HEADER_PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


@pytest.fixture(scope="module")
def compiler_view(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    body = [f'    Fn<decltype(&{n})>::print("{n}");' for n in _lib.SIGNATURES]
    for n, cls in _lib.STRUCTS.items():
        body.append(f'    std::printf("S {n} %zu", sizeof({n}));' + "".join(f" FIELD({n}, {f});" for f, _ in cls._fields_)
                    + ' std::puts("");')
    body += [f'    std::printf("C {n} %lld\\n", (long long)(HSP_{n}));' for n in _lib.CONSTANTS]
    d = tmp_path_factory.mktemp("abi")
    (d / "abi.cpp").write_text(PROGRAM.replace("@BODY@", "\n".join(body)))
    subprocess.run([cxx, "-std=c++17", "-I", os.path.dirname(_lib.HEADER_PATH), str(d / "abi.cpp"), "-o", str(d / "abi")],
                   check=True)
    out = subprocess.run([str(d / "abi")], check=True, capture_output=True, text=True).stdout.splitlines()
    return {k: [ln.split()[1:] for ln in out if ln.startswith(k + " ")] for k in "FSC"}


def test_prototypes_are_the_compilers(compiler_view):
    got = {f[0]: f[1:] for f in compiler_view["F"]}
    assert len(got) == len(compiler_view["F"]) == len(_lib.SIGNATURES) == len(set(re.findall(r"\b(hsp_[a-z0-9_]+)\s*\(", _header_text())))
    for name, (res, args) in _lib.SIGNATURES.items():
        assert [_code(res)] + [_code(a) for a in args] == got[name], name


def test_structs_are_the_compilers(compiler_view):
    got = {s[0]: s[1:] for s in compiler_view["S"]}
    assert len(got) == len(_lib.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", _header_text()))
    for name, cls in _lib.STRUCTS.items():
        size, *fields = got[name]
        assert getattr(_lib, name) is cls and ctypes.sizeof(cls) == int(size), name
        want = [f"{f}:{getattr(cls, f).offset}:{getattr(cls, f).size}:{_code(ct)}" for f, ct in cls._fields_]
        assert want == fields, name


def test_constants_are_the_compilers(compiler_view):
    got = {c[0]: int(c[1]) for c in compiler_view["C"]}
    assert len(got) == len(_lib.CONSTANTS) == len(re.findall(r"^\s*#\s*define\s+HSP_\w+[ \t]+\S", _header_text(), flags=re.M))
    assert got == _lib.CONSTANTS
    assert all(getattr(_lib, n) == v for n, v in got.items())


STRUCT = "typedef struct HspPair { int a, b; } HspPair;\n"


@pytest.mark.parametrize("text, quoted", [
    ("int hsp_f(int n, widget_t w);", "int hsp_f(int n, widget_t w)"),                    # an unknown type name
    (STRUCT + "int hsp_f(HspPair p);", "int hsp_f(HspPair p)"),                           # a struct by value
    (STRUCT + "HspPair hsp_f(int n);", "HspPair hsp_f(int n)"),
    ("#define HSP_RATIO 1.5\nint hsp_f(int n);", "#define HSP_RATIO 1.5"),                # a non-integer beside an HSP_ name
    ("#define HSP_TWICE(x) (2 * (x))\n", "#define HSP_TWICE(x) (2 * (x))"),
    ("#pragma once\nint hsp_f(int n);", "#pragma once"),                                  # an unknown directive
    ("int hsp_f(int n);\nint hsp_g(const float *x, int n)\n", "int hsp_g(const float *x, int n)"),   # cut off before `;`
    ("typedef struct HspBad { int n; widget_t w; } HspBad;", "typedef struct HspBad { int n; widget_t w; } HspBad"),
], ids=["type", "by-value", "by-value-return", "define-float", "define-macro", "directive", "cut-off", "field-type"])
def test_reader_refuses_and_quotes(text, quoted):
    with pytest.raises(_lib.HspError, match=re.escape(quoted)):
        _lib.parse_header(text)


def test_reader_accepts_the_forms_it_refuses_nothing_of():
    """the refusals above are not the reader refusing everything: the same texts, mended, parse"""
    protos, structs, consts = _lib.parse_header(
        "#define HSP_NEG (-7)\n" + STRUCT + "const char *hsp_f(const HspPair *p, const float *const *x, int out[4], long long n);")
    assert protos == {"hsp_f": (ctypes.c_char_p, [ctypes.c_void_p] * 3 + [ctypes.c_longlong])}
    assert structs == {"HspPair": [("a", ctypes.c_int), ("b", ctypes.c_int)]} and consts == {"HSP_NEG": -7}


def test_missing_header_names_its_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "hsp.h"))
    with pytest.raises(_lib.HspError, match=re.escape(str(tmp_path / "include" / "hsp.h"))):
        _lib._read_header()
