"""ctypes binding of libhsp.so, derived from include/hsp.h at import: prototypes, structs and constants are read from the
header, nothing of it is restated here.  Loaded lazily on the first device op; a missing library is a hard error -- there is no
fallback path."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# HSP_LIB=<path> loads another build of the same ABI (profiling variants); default: the in-tree library
LIB_PATH = os.environ.get("HSP_LIB") or os.path.join(_HERE, "libhsp.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hsp.h")
_lib = None


class HspError(RuntimeError):
    pass


# the closed table of scalar types the ABI passes by value; a fixed-width type joins it when the header comes to need it
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
            "unsigned long long": ctypes.c_ulonglong, "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32,
            "uint16_t": ctypes.c_uint16, "uint8_t": ctypes.c_uint8, "int8_t": ctypes.c_int8}
_POINTEES = ("void", "char")            # further type names that may stand under a `*` only
_STARS = r"((?:\s*\*)*)\s*"
_DECL = re.compile(r"(.+?)" + _STARS + r"(\w+)\s*(\[\w*\])?", re.S)


def parse_header(text):
    """(prototypes, structs, constants) of the text of include/hsp.h: name -> (restype, [argtypes]), struct name -> [(field,
    ctype)], HSP_NAME -> int.  Narrow and strict by design: it accepts the forms the header uses and raises ``HspError`` with the
    offending text on anything else, so a declaration it does not understand fails at import instead of going unbound."""
    protos, structs, consts, types = {}, {}, {}, dict(_SCALARS)

    def bad(why, what):
        return HspError(f"include/hsp.h: {why}: `{' '.join(what.split())}`")

    def ctype(base, ptr, whole):
        """the ctypes type of `base` with (ptr) or without a `*` / `[]`, in the declaration `whole`"""
        base = " ".join(base.split())
        if base not in types and base not in structs and not (ptr and base in _POINTEES):
            raise bad(f"unknown type name `{base}`", whole)
        if ptr:
            return ctypes.c_void_p
        if base in structs:
            raise bad(f"struct `{base}` passed by value", whole)
        return types[base]

    def declarator(piece, whole):
        m = _DECL.fullmatch(piece.strip())
        if not m:
            raise bad("declaration not understood", whole)
        base, stars, name, array = m.groups()
        return base, name, ctype(base, bool(stars.strip() or array), whole)

    def fields(body, whole):
        out = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            base, name, ct = declarator(first, whole)
            out.append((name, ct))
            for piece in more:                  # `const void *A1, *B1;`: each declarator carries its own `*`
                m = re.fullmatch(_STARS + r"(\w+)", piece.strip())
                if not m:
                    raise bad("declaration not understood", whole)
                out.append((m.group(2), ctype(base, bool(m.group(1).strip()), whole)))
        return out

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    code, guard, in_cpp = [], None, False
    for line in text.split("\n"):
        s = " ".join(line.split())
        if not s.startswith("#"):
            if in_cpp and s not in ("", 'extern "C" {', "}"):
                raise bad("unexpected text in the __cplusplus block", s)
            if not in_cpp:
                code.append(line)
            continue
        m = re.fullmatch(r"# ?define (HSP_\w+) (\(-?\d+\)|-?\d+)", s)
        if m:
            consts[m.group(1)] = int(m.group(2).strip("()"))
        elif re.fullmatch(r"# ?ifndef \w+", s) and guard is None:
            guard = s.split()[-1]
        elif s == "#ifdef __cplusplus":
            in_cpp = True
        elif s == "#endif":
            in_cpp = False
        elif not (re.fullmatch(r"# ?include <\w+\.h>", s) or (guard and re.fullmatch(r"# ?define " + guard, s))):
            raise bad("directive not understood", s)

    *stmts, rest = re.sub(r"\{[^{}]*\}", lambda m: m.group(0).replace(";", "\0"), "\n".join(code)).split(";")
    if rest.strip():
        raise bad("declaration cut off before `;`", rest)
    for st in (s.replace("\0", ";").strip() for s in stmts):       # st: the declaration as written, for messages
        nc = re.sub(r"\bconst\b", " ", st)                          # `const` does not change how a value is passed
        m = re.fullmatch(r"typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)", nc, re.S)
        if m:
            if m.group(1) != m.group(3) or m.group(1) in structs:
                raise bad("struct tag and typedef name differ, or the struct is declared twice", st)
            structs[m.group(1)] = fields(m.group(2), st)
            continue
        if nc.startswith("typedef"):
            _, name, ct = declarator(nc[len("typedef"):], st)
            types[name] = ct
            continue
        head, _, params = nc.partition("(")
        m = _DECL.fullmatch(head.strip())
        if not m or m.group(4) or not params.endswith(")") or "{" in st or m.group(3) in protos:
            raise bad("declaration not understood, or declared twice", st)
        ret, stars, name, _ = m.groups()
        if re.fullmatch(r"const\s+char\s*\*\s*\w+", st.partition("(")[0].strip()):
            res = ctypes.c_char_p
        else:
            res = ctype(ret, bool(stars.strip()), st)
        protos[name] = (res, [] if params[:-1].strip() == "void" else [declarator(p, st)[2] for p in params[:-1].split(",")])
    return protos, structs, consts


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise HspError(f"{HEADER_PATH}: the ABI header libhsp.so is bound from cannot be read ({e})") from None


# SIGNATURES: name -> (restype, argtypes) of every entry point.  STRUCTS: name -> the struct's ctypes class.  CONSTANTS: the header's
# HSP_<NAME> integers under <NAME>.  Structs and constants are module attributes too (HspGemmCall, GEMM_ROUTE_X3, ERR_LAUNCH, ...).
SIGNATURES, _fields, _consts = _read_header()
STRUCTS = {n: type(n, (ctypes.Structure,), {"_fields_": f, "__doc__": f"include/hsp.h: {n}"}) for n, f in _fields.items()}
CONSTANTS = {n[len("HSP_"):]: v for n, v in _consts.items()}
globals().update(STRUCTS)
globals().update(CONSTANTS)


def lib():
    """The loaded libhsp.so with argtypes set.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HspError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C hs_pose_amd/csrc`). "
                "hs_pose_amd has no CPU / eager fallback.")
        # torch first: its wheel carries its own libamdhip64.so, and libhsp.so's NEEDED entry (same soname) must resolve to THAT copy.
        # Loaded before torch, libhsp.so pulls in /opt/rocm's runtime; torch then brings a second one, the device is initialised in one
        # and the kernels are registered in the other: every launch fails with "no ROCm-capable device is detected" (seen when
        # build() and smoke() ran in one process).
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        L = lib()
        msg = L.hsp_error_string(rc).decode()
        hip = L.hsp_last_hip_error().decode()
        raise HspError(f"{what} failed: {msg} (code {rc})" + (f" [hip: {hip}]" if hip and rc == CONSTANTS["ERR_LAUNCH"] else ""))
