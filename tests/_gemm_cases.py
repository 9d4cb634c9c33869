"""The case table of the dense-product reference tests: the smallest shapes on each side of each pick rule of csrc/gemm.hip,
with the plan each is meant to enter, and (ROUTES) product calls with the kernel family hsp_gemm_route sends each to.  tests/test_gemm_plans_host.py asserts the plans on the CPU (the plan queries are host
code); tests/test_gpu_gemm_reference.py asserts them again and runs the kernels."""
import ctypes
from collections import namedtuple

from hs_pose_amd import _lib

KB1, KB4, BF16, X3 = _lib.WGRAD_FORM_F32_KB1, _lib.WGRAD_FORM_F32_KB4, _lib.WGRAD_FORM_BF16, _lib.WGRAD_FORM_X3
FOLD_MAX_WGRAD = _lib.FOLD_MAX_WGRAD


def _c4(m):
    return (m + 3) & ~3


def _c8(m):
    return (m + 7) & ~7


# entry: "f32" hsp_wgrad_f32, "bf16" hsp_wgrad_bf16, "rbf16" hsp_wgrad_ragged_bf16.  lda / ldb: the operands' row pitches in
# elements; al16: both operands start on 16 bytes.  form: the plan the case is placed for; want: further facts of the plan
# ("slices": K slices, "parts": partial sums, "past": the last slice starts at or past K, "fewer": wgrad_bf16_pick's cost rule
# took fewer slices than its first choice, "full": it kept the first choice)
W = namedtuple("W", "entry M N K lda ldb al16 form want")


def _w(entry, M, N, K, lda=None, ldb=None, al16=1, form=None, **want):
    return W(entry, M, N, K, M if lda is None else lda, N if ldb is None else ldb, al16, form, want)


WGRAD = (
    # fp32-MFMA form, a wave per (tile, slice): one tile and K too short for 8 slices of 32 rows; pitches 2 * odd (x3 declines)
    [_w("f32", 64, 64, K, 66, 66, form=KB1, slices=s) for K, s in ((1, 1), (2, 1), (15, 1), (16, 1), (17, 1), (37, 1), (255, 2))]
    + [
        _w("f32", 64, 64, 256, 66, 66, form=KB4, slices=8, parts=2),              # K / 32 == 8: the first KB = 4 shape
        _w("f32", 64, 64, 300, 66, 66, form=KB4, slices=8, parts=2, past=True),   # 7 slices of 48 rows + one that starts past K
        _w("f32", 128, 192, 4113, 130, 194, form=KB4, slices=88, parts=22),
        _w("f32", 320, 832, 300, 322, 834, form=KB1, slices=3),                    # 65 tiles: over the 64-tile rule
        _w("f32", 128, 384, 257, form=KB4, slices=8),                              # three 128-tiles: x3 declines by its tile count
        _w("f32", 128, 512, 1000, 130, 514, form=KB4, slices=24),                  # four tiles, but pitches off 16 bytes
        _w("f32", 128, 512, 65, 132, 516, al16=0, form=KB1, slices=1),             # four tiles, pitches fine, base pointers off 16 bytes
    ]
    # x3 form: exactly four 128-tiles, at the K edges of its 32-row blocks and of wgrad_bf16_pick's 256 rows per slice
    + [_w("f32", 128, 512, K, form=X3, slices=s) for K, s in ((1, 1), (63, 1), (64, 1), (65, 1), (256, 1), (257, 2), (1000, 4))]
    + [
        _w("f32", 256, 256, 257, form=X3, slices=2),
        _w("f32", 128, 512, 257, 132, 516, form=X3, slices=2),                     # a pitch pad the form admits (multiples of 4)
        _w("f32", 256, 256, 65, 260, 260, form=X3, slices=1),
        _w("f32", 64, 512, 1000, form=X3, slices=4),                               # M an odd multiple of 64: half a row tile
        _w("f32", 192, 256, 513, form=X3, slices=3),
    ]
    # ragged M on the dense pitch and on a wider one
    + [_w("f32", M, 512, 257, _c4(M) + pad, form=X3, slices=2) for M in (129, 130, 191, 771) for pad in (0, 4)]
    + [
        _w("f32", 129, 1408, 6144, 132, form=X3, fewer=True),                      # 22 tiles x 24 slices = 528 workgroups: one slice fewer
        _w("f32", 129, 1024, 8192, 132, form=X3, full=True, slices=32),            # 16 tiles divide 512: the first choice stays
    ]
    # bf16 rows on the bf16 MFMA
    + [_w("bf16", 128, 128, K, form=BF16, slices=s) for K, s in ((1, 1), (63, 1), (64, 1), (65, 1), (256, 1), (257, 2), (1000, 4))]
    + [
        _w("bf16", 256, 128, 257, 264, 136, form=BF16, slices=2),
        _w("bf16", 128, 128, 65, 136, 136, form=BF16, slices=1),                   # a pitch pad the form admits (multiples of 8)
        _w("bf16", 128, 256, 1000, 136, 264, form=BF16, slices=4),
        _w("bf16", 64, 128, 257, form=KB4, slices=8),                              # M = 64: the fp32 MFMA on bf16 storage
        _w("bf16", 128, 128, 257, 132, 128, form=KB4, slices=8),                   # lda % 8 != 0: likewise
        _w("bf16", 128, 128, 37, 130, 130, al16=0, form=KB1, slices=1),
    ]
    + [_w("rbf16", M, 128, 257, _c8(M) + pad, form=BF16, slices=2) for M, pad in ((129, 0), (136, 0), (136, 8), (1286, 0))]
)

# ragged bf16 rows hsp_wgrad_ragged_bf16 declines (ops.wgrad used to send them there): fewer than 128 output rows, base pointers off
# 16 bytes, N off the 128-wide tiles; and a pitch off 16 bytes
WGRAD_DECLINED = [_w("rbf16", 100, 128, 257, 104), _w("rbf16", 129, 128, 257, 136, al16=0), _w("rbf16", 129, 192, 257, 136),
                  _w("rbf16", 129, 128, 257, 132)]

# hsp_wgrad_partial_pair_f32: (M0, N0, K0, M1, N1, K1, one launch, shrunk)
PAIRS = [
    (128, 128, 256, 128, 128, 256, True, False),
    (128, 128, 2056, 128, 128, 2056, True, False),
    (128, 128, 16448, 128, 128, 16448, True, False),      # 2 x 208 workgroups: inside one round of 512 as it is
    (128, 128, 16448, 128, 256, 16448, True, True),       # 208 + 416 workgroups: the shrink loop
    (128, 128, 300, 320, 832, 300, False, False),         # the second problem is not K-sliced: two launches
]


def wgrad_plan(L, c):
    out = (ctypes.c_int * 4)()
    rc = L.hsp_wgrad_plan(c.M, c.N, c.K, 2 if "bf16" in c.entry else 4, c.al16, c.lda, c.ldb, 1 if c.entry == "rbf16" else 0, out)
    return rc, list(out)


def pair_plan(L, p):
    out = (ctypes.c_int * 7)()
    rc = L.hsp_wgrad_pair_plan(*p[:6], out)
    return rc, list(out)


def check_wgrad_plan(L, c):
    """the plan a case enters, and the facts every weight-gradient kernel relies on; returns (form, slices, rows per slice, partials)"""
    rc, (form, sk, ks, parts) = wgrad_plan(L, c)
    assert rc == 0, f"{c}: declined ({rc})"
    assert form == c.form, f"{c}: form {form}"
    assert ks % 16 == 0 and ks > 0, f"{c}: slice of {ks} rows"
    if form in (BF16, X3):
        assert ks % 64 == 0 and (sk - 1) * ks < c.K <= sk * ks and parts == sk, f"{c}: {sk} x {ks}"
    elif form == KB4:
        assert sk % 4 == 0 and parts == sk // 4 and c.K <= sk * ks, f"{c}: {sk} x {ks}"
    else:
        assert parts == sk and (sk - 1) * ks < c.K <= sk * ks, f"{c}: {sk} x {ks}"
    assert parts * (c.M * c.N + c.N) * 4 <= L.hsp_wgrad_workspace_bytes(c.M, c.N, c.K), f"{c}: {parts} partials overrun the workspace"
    w = c.want
    if "slices" in w:
        assert sk == w["slices"], f"{c}: {sk} slices"
    if "parts" in w:
        assert parts == w["parts"], f"{c}: {parts} partials"
    if w.get("past"):
        assert (sk - 1) * ks >= c.K, f"{c}: no slice starts past K"
    if "fewer" in w or "full" in w:
        tiles = ((c.M + 127) // 128) * (c.N // 128)
        first = min(-(-512 // tiles), (c.K + 255) // 256, 128)                        # wgrad_bf16_pick's first choice
        if w.get("fewer"):
            assert tiles * first > 512 >= tiles * sk, f"{c}: {tiles} tiles x {sk} slices (first choice {first})"
        else:
            assert sk == first and tiles * first <= 512, f"{c}: {tiles} tiles x {sk} slices (first choice {first})"
    return form, sk, ks, parts


def check_pair_plan(L, p):
    M0, N0, K0, M1, N1, K1, one, shrunk = p
    rc, (o, sk0, ks0, sk1, ks1, b0, b1) = pair_plan(L, p)
    assert rc == 0 and bool(o) == one, f"{p}: rc {rc}, one launch {o}"
    if not one:
        return None
    for M, N, K, sk, ks, b in ((M0, N0, K0, sk0, ks0, b0), (M1, N1, K1, sk1, ks1, b1)):
        assert sk % 4 == 0 and ks % 16 == 0 and sk * ks >= K and b == (M // 64) * (N // 64) * (sk // 4)
        assert (sk // 4) * (M * N + N) * 4 <= L.hsp_wgrad_workspace_bytes(M, N, K), f"{p}: {sk // 4} partials overrun the workspace"
        alone = (ctypes.c_int * 4)()
        assert L.hsp_wgrad_plan(M, N, K, 4, 0, M + 2, N + 2, 0, alone) == 0 and alone[0] == KB4
        assert (sk < alone[1]) == shrunk, f"{p}: {sk} slices in the pair, {alone[1]} alone"
    assert (b0 + b1 <= 512) or not shrunk
    return sk0, ks0, sk1, ks1


# ---- hsp_gemm_route: product calls and the kernel family each goes to ----------------------------------------------------------
NONE, SMALL, X3R, X3_BN, WAVE, TILE = (getattr(_lib, "GEMM_ROUTE_" + r) for r in ("NONE", "SMALL_ROWS", "X3", "X3_BN", "WAVE", "TILE"))
BN_OUT, BN_LIN = _lib.GEMM_BN_OUT, _lib.GEMM_BN_LINEAR

# lay: the weight layouts, "nt" (N,K) | "nn" (K,N), one per source ("nn+nt": two sources); epi: b bias, r residual, c per-cloud
# bias, x the xyz3 rider; off: None, "C0" (no result yet: the caller allocates it dense) or (operand, "ptr" | "ld"): that operand's
# base address / row pitch moved off 16 bytes (by 4 bytes / one element); x3: ops.GEMM_X3; es: bytes per element
G = namedtuple("G", "M N K1 K2 lay epi want alpha rpc off relu bn x3 es")


def _g(M, N, K1, K2=0, lay="nt", epi="", want=None, alpha=1.0, rpc=0, off=None, relu=False, bn=0, x3=1, es=4):
    return G(M, N, K1, K2, lay + ("+nt" if K2 and "+" not in lay else ""), epi, want, alpha, rpc, off, relu, bn, x3, es)


def _network(B, N0):
    """every dense product of the training step at B clouds of N0 points: the surface layer, the four HS layers (fm = X W + b; out
    = x Wste^T + F Wa^T + F + t[cloud], alone and with the BatchNorm partials; g Wa; gX = g Wste + gfm W^T; the per-cloud t = fg
    Wb^T and its input gradient), the heads' Conv1d(k=1) layers on 1286 / 1289 / 771 / 259 and narrower inputs (forward, with
    the BatchNorm partials, input gradient, input gradient accumulated into a residual) and the per-cloud towers.  An epilogue
    with fewer than 128 tiles of 64 rows keeps a product off x3; more than 512 BatchNorm row tiles keep the partials off."""
    N1, N2 = (N0 + 3) // 4, (N0 + 3) // 4 // 4
    rows = [_g(B * N0, 128, 128, epi="rcx", rpc=N0, relu=True, want=WAVE)]
    for Np, Cin, C in ((N0, 128, 128), (N1, 128, 256), (N1, 256, 256), (N2, 256, 512)):
        M = B * Np
        epi_x3 = -(-M // 64) * (C // 128) >= 128
        out = X3R if epi_x3 else TILE
        rows += [
            _g(M, 8 * C, Cin, lay="nn", epi="b", want=X3R),
            _g(M, C, Cin, C, epi="rc", rpc=Np, want=out),
            _g(M, C, Cin, C, epi="rc", rpc=Np, bn=BN_OUT, off="C0", want=X3_BN if epi_x3 and -(-M // 64) <= 512 else out),
            _g(M, C, C, lay="nn", want=X3R if M >= 4096 else WAVE),
            _g(M, Cin, C, 8 * C, lay="nn+nt", want=X3R),
            _g(B, C, C, want=SMALL),
            _g(B, C, C, lay="nn", alpha=1.0 / Np, off="C0", want=SMALL),
        ]
    M = B * N0
    for K, N in ((1286, 1024), (1289, 1024), (1286, 512), (771, 512), (259, 512), (1024, 256), (512, 512), (512, 256), (256, 128)):
        rows += [
            _g(M, N, K, epi="b", off="C0", want=X3R),
            _g(M, N, K, epi="b", off="C0", bn=BN_LIN, want=X3_BN if -(-M // 128) <= 512 else X3R),
            _g(M, K, N, lay="nn", want=X3R),
            _g(M, K, N, lay="nn", epi="r", want=X3R),
        ]
    return rows + [_g(B, 256, 256, epi="b", want=TILE), _g(B, 4, 256, epi="b", want=TILE), _g(M, 3, 128, epi="b", want=TILE)]


_OUT = dict(M=16448, N=128, K1=128, K2=128, epi="rc", rpc=1028)          # the layer's out product, every operand in use
ROUTES = (
    _network(16, 1028) + _network(64, 4096)
    # small rows: <= 16 rows, or <= 64 on its matrix-core form (K a multiple of 128; "nt" needs 16-byte rows); K <= 2048; no rider
    + [_g(16, 64, 1000, want=SMALL), _g(17, 64, 1000, want=TILE), _g(17, 64, 1024, want=SMALL), _g(64, 64, 128, want=SMALL),
       _g(65, 64, 128, want=TILE), _g(17, 64, 128, off=("A1", "ptr"), want=TILE), _g(17, 64, 128, off=("B1", "ld"), want=TILE),
       _g(17, 64, 128, lay="nn", off=("A1", "ptr"), want=SMALL), _g(16, 64, 2048, want=SMALL), _g(16, 64, 2049, want=TILE),
       _g(16, 64, 128, epi="b", want=TILE), _g(16, 64, 128, 128, want=TILE),
       # ("nn" off the matrix-core form: the rows and 3072 partial sums share 64 KB of LDS -- ops.gemm_own used to send the
       # second there, where the entry point declines it)
       _g(16, 64, 832, lay="nn", want=SMALL), _g(16, 64, 833, lay="nn", want=TILE), _g(16, 64, 1000, lay="nn", want=TILE)]
    # x3: from 256 rows on; hsp_gemm_x3_supported's two clauses (128 tiles of 64 rows, or 32 k-blocks); with an epilogue 128 tiles
    + [_g(255, 4096, 128, want=WAVE), _g(256, 4096, 128, want=X3R), _g(8128, 128, 1024, want=X3R), _g(8128, 128, 992, want=TILE),
       _g(8129, 128, 992, want=X3R), _g(8128, 128, 1024, epi="b", want=TILE), _g(8129, 128, 1024, epi="b", want=X3R),
       _g(256, 4096, 128, x3=0, want=WAVE), _g(256, 4096, 128, epi="rcx", rpc=64, want=WAVE), _g(8129, 63, 1024, want=TILE),
       # a residual alone: one source and alpha == 1 (ops.gemm_own used to send any alpha there)
       _g(16448, 1286, 1024, lay="nn", epi="r", want=X3R), _g(16448, 1286, 1024, lay="nn", epi="r", alpha=0.5, want=TILE),
       _g(16448, 1286, 512, 512, lay="nn+nt", epi="r", want=TILE), _g(16448, 1286, 1024, epi="c", rpc=1028, want=X3R),
       _g(16448, 1286, 1024, epi="br", want=TILE)]
    # the wave kernel (x3 off): K1 + K2 <= 512, M N >= 512 K, clouds of >= 64 rows, its seven forms, N and K multiples of 32
    + [_g(4096, 128, 512, x3=0, want=WAVE), _g(4096, 128, 544, x3=0, want=TILE), _g(4096, 128, 256, 256, x3=0, epi="rc", rpc=64, want=WAVE),
       _g(4096, 128, 256, 288, x3=0, epi="rc", rpc=64, want=TILE), _g(4095, 128, 128, x3=0, want=TILE), _g(4097, 128, 128, x3=0, want=WAVE),
       _g(4096, 128, 128, 128, x3=0, epi="rc", rpc=63, want=TILE), _g(4096, 128, 128, 128, x3=0, epi="rc", rpc=64, want=WAVE),
       _g(4096, 128, 128, x3=0, epi="r", want=TILE), _g(4096, 128, 128, 128, x3=0, lay="nt+nn", want=TILE),
       _g(4096, 128, 128, x3=0, relu=True, want=TILE), _g(4096, 160, 128, x3=0, want=WAVE), _g(4096, 144, 128, x3=0, want=TILE),
       _g(4096, 128, 144, x3=0, want=TILE)]
    # an operand off 16 bytes: x3 needs its activation rows there and nothing else, the wave kernel every operand
    + [_g(**_OUT, want=X3R), _g(**_OUT, x3=0, want=WAVE)]
    + [_g(**_OUT, off=(o, k), want=TILE if o in ("A1", "A2") else X3R) for o in ("A1", "B1", "A2", "B2", "resid", "C") for k in ("ptr", "ld")]
    + [_g(**_OUT, off=(o, k), x3=0, want=TILE) for o in ("A1", "B1", "A2", "B2", "resid", "C") for k in ("ptr", "ld")]
    # the BatchNorm partials: the out product from clouds of 64 rows on, a Linear from 256 rows on, 512 row tiles at most
    + [_g(16384, 128, 128, 128, epi="rc", rpc=64, bn=BN_OUT, want=X3_BN), _g(16128, 128, 128, 128, epi="rc", rpc=63, bn=BN_OUT, want=X3R),
       _g(32768, 128, 128, 128, epi="rc", rpc=64, bn=BN_OUT, want=X3_BN), _g(32769, 128, 128, 128, epi="rc", rpc=64, bn=BN_OUT, want=X3R),
       _g(16384, 128, 128, 128, epi="rc", rpc=64, bn=BN_OUT, relu=True, want=X3R), _g(16384, 128, 128, 128, epi="rc", rpc=64, bn=BN_OUT, x3=0, want=WAVE),
       _g(256, 4096, 128, epi="b", bn=BN_LIN, want=X3_BN), _g(255, 4096, 128, epi="b", bn=BN_LIN, want=WAVE),
       _g(65536, 1024, 128, epi="b", bn=BN_LIN, want=X3_BN), _g(65537, 1024, 128, epi="b", bn=BN_LIN, want=X3R),
       _g(16448, 1024, 1286, bn=BN_LIN, want=X3R)]
    # bf16 rows: the tile kernel, (N,K) weights only; two (K,N) weights: x3 (its planes are (N,K) whatever the weight) or no kernel
    + [_g(16448, 128, 128, es=2, want=TILE), _g(16448, 128, 128, es=2, lay="nn", want=NONE), _g(16448, 128, 128, 128, lay="nn+nn", want=X3R),
       _g(16448, 128, 128, 128, lay="nn+nn", x3=0, want=NONE),
       _g(16448, 128, 128, es=2, off=("A1", "ld"), want=NONE)]
)


def gemm_call(c):
    """the HspGemmCall of a ROUTES row: operands at made-up addresses on pitches rounded up to 16 bytes"""
    from hs_pose_amd._lib import HspGemmCall
    per16 = 16 // c.es
    lays = [int(x == "nn") for x in c.lay.split("+")] + [0]

    def op(name, cols, addr):
        ld = -(-cols // per16) * per16
        if c.off is not None and c.off[0] == name:
            addr, ld = (addr + 4, ld) if c.off[1] == "ptr" else (addr, ld + 1)
        return addr, ld

    (a1, lda1), (b1, ldb1) = op("A1", c.K1, 0x100000), op("B1", c.N if lays[0] else c.K1, 0x200000)
    (a2, lda2), (b2, ldb2) = (op("A2", c.K2, 0x300000), op("B2", c.N if lays[1] else c.K2, 0x400000)) if c.K2 else ((None, 0), (None, 0))
    r, ldr = op("resid", c.N, 0x500000) if "r" in c.epi else (None, 0)
    out, ldc = (None, c.N) if c.off == "C0" else op("C", c.N, 0x600000)
    return HspGemmCall(a1, b1, a2, b2, r, out, c.M, c.N, c.K1, c.K2, lays[0], lays[1], c.es, lda1, ldb1, lda2, ldb2, ldr, ldc,
                       "b" in c.epi, "c" in c.epi, "x" in c.epi, c.relu, c.alpha == 1.0, c.rpc, c.bn, c.x3)
