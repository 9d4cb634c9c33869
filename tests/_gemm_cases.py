"""The case table of the dense-product reference tests: the smallest shapes on each side of each pick rule of csrc/gemm.hip,
with the plan each is meant to enter.  tests/test_gemm_plans_host.py asserts the plans on the CPU (the plan queries are host
code); tests/test_gpu_gemm_reference.py asserts them again and runs the kernels."""
import ctypes
from collections import namedtuple

KB1, KB4, BF16, X3 = 0, 1, 2, 3          # include/hsp.h: HSP_WGRAD_FORM_*
FOLD_MAX_WGRAD = 24                       # include/hsp.h: HSP_FOLD_MAX_WGRAD


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
