"""tools/x3_isa_report.py [source.hip] -- what hipcc made of the x3 tile kernels, without a GPU: per instantiation of
gemm_x3_kernel the VGPRs, the scratch bytes, the spill count and the number of full queue drains (``s_waitcnt vmcnt(0)``)
after the kernel's last barrier, i.e. in its epilogue.  Compiles hs_pose_amd/csrc/gemm_x3.hip (or the given file) to
assembly with the Makefile's flags.  DESIGN.md section 4 quotes its table."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hs_pose_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--cuda-device-only", "-S"]


def report(src):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "x3.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + [src, "-o", asm])
        text = open(asm).read()
    syms = re.findall(r"^(_Z\w+):", text, re.M)
    try:
        names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    except OSError:                                   # no binutils: the mangled names carry the same template arguments
        names = syms
    demangled = dict(zip(syms, names))
    rows = []
    for m in re.finditer(r"^(_Z\w*gemm_x3_kernel\w+):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        sym, body, meta = m.groups()
        tail = body.rsplit("s_barrier", 1)[-1]
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        spill = re.search(r"\.name:\s+%s\n.*?\.vgpr_spill_count:\s+(\d+)" % re.escape(sym), text, re.S)
        rows.append((demangled.get(sym, sym).split("(")[0].replace("void hsp::", ""), vgpr, scratch,
                     int(spill.group(1)) if spill else -1, len(re.findall(r"s_waitcnt vmcnt\(0\)", body)),
                     len(re.findall(r"s_waitcnt vmcnt\(0\)", tail))))
    print(f"{'kernel':48s} {'vgpr':>5s} {'scratch':>8s} {'spills':>7s} {'drains':>7s} {'after last barrier':>19s}")
    for r in sorted(rows):
        print(f"{r[0]:48s} {r[1]:5d} {r[2]:8d} {r[3]:7d} {r[4]:7d} {r[5]:19d}")
    return rows


if __name__ == "__main__":
    report(sys.argv[1] if len(sys.argv) > 1 else os.path.join(CSRC, "gemm_x3.hip"))
