"""GPU: the weight-gradient family of csrc/gemm.hip (hsp_wgrad_f32 on its fp32-MFMA forms and on the x3 form, hsp_wgrad_bf16,
hsp_wgrad_ragged_bf16, the pair launch with its column-sum rider, hsp_wgrad_fold, hsp_step_fold) and the row products of
csrc/gemm_rows.hip (hsp_gemm_rows_f32, _bf16, _acc_bf16: C = alpha (A1 op(B1) + A2 op(B2)) + bias + resid + xyz3 . w3 +
cloud_bias[row // rows_per_cloud], T with the absolute value of every addend), the same contract on hsp_gemm_x3_f32 (tile kernel,
panel kernel, split-K with both paths of its fold) and hsp_gemm_wave_f32 (every instantiated form and tile configuration), and the
per-cloud products hsp_small_rows_f32 / hsp_small_outer_f32 / hsp_small_pair_f32, against a plain float64 reference on the CPU,
element by element, at the edges of the dispatch:

    C[m][n]   = sum_k A[k][m] B[k][n]        colsum[n] = sum_k B[k][n]            (stored values; bf16 widened exactly)
    T[m][n]   = sum_k |A[k][m]| |B[k][n]|    Tcs[n]    = sum_k |B[k][n]|
    |got - want| <= A * 2^-24 * T            per element: no floor, no norm, no outlier allowance

A is 4x the worst ratio err / (2^-24 T) of the fp32 torch composition (torch.mm in fp32 plus the same epilogue) on the same cases
and data sets, rounded up to a power of two, per family (test_fp32_composition_sets_A* hold that rule, on the CPU).  A bf16 output
gets a further 2^-8 |want|, its one rounding.

Operands (seeded torch.Generator): randn * 2^(row exponent) * 2^(column exponent), exponents drawn from [-12, 12], so the three
bf16 slices of the x3 form and the split-K partials see 48 binades of range; and a second data set with forced cancellation: the
second half of the K rows repeats the first, permuted, with A negated and perturbed by 2^-10 relative, so |want| << T.

Moats: every operand is a view (leading elements, a row pitch wider than the row where the form allows one) of a parent filled
with NaN; every output is a NaN-prefilled view (ldc = N + 1) of a parent filled with a sentinel; every workspace is passed at
exactly the size hsp_wgrad_workspace_bytes returns with a sentinel band behind it.  After the call the output holds no NaN the
reference lacks and the parents' sentinels and the band are intact bit for bit.

Every case asserts the plan it enters (hsp_wgrad_plan, hsp_wgrad_pair_plan, hsp_gemm_rows_plan, hsp_gemm_x3_plan,
hsp_gemm_wave_plan_info: the dispatch decides by the same functions; the weight-gradient table and its plan facts are
tests/_gemm_cases.py, held on the CPU by tests/test_gemm_plans_host.py).

The folds are fed partial sums the test writes itself and must equal, bit for bit, the documented order evaluated in fp32 on the
CPU: group g = 0..3 adds the partials g, g+8, ... and g+4, g+12, ... in two accumulators, adds the second to the first, and the
four groups are added in ascending order.

Measured ratios err / (2^-24 T), worst over the cases and data sets of this file (composition on the CPU, where torch.mm's blocking
makes the figure differ by machine; kernels on an MI355X); the same table is in DESIGN.md section 2.0b:
    composition:  C = A^T B 13.1 ... 18.4   column sum 3.5   gemm_rows products with their epilogue 14.1 ... 14.8
                  gemm_x3 cases 17.2   wave cases 9.5   per-cloud products 10.3
                  ->  A = 128 (weight gradients), A_SUM = 16, A_ROWS = 64, A_X3 = 128, A_WAVE = 64, A_SMALL = 64.
                  The project's A = 32 does not hold under its own rule here: with 48 binades of range a few terms carry a sum.
    kernels:      wgrad fp32 MFMA KB = 1  11.4 (colsum 3.7)    KB = 4  7.6 (colsum 2.0)    pair launch 4.1 (rider 0.8)
                  wgrad x3  16.8 (colsum 2.9): the dropped cross terms are each ~2^-24 of a term and ride on the chain's own rounding
                  wgrad bf16 MFMA  6.3 (colsum 2.2)    step fold, direction entries 5.0 of their (nparts + 16) bound's unit
                  gemm_rows fp32  26.2 (129 x 129 <- 1025 "nn" rows run UNSPLIT: one fma chain of 1025 terms; 9.7 when split in 7)
                  gemm_rows bf16  7.9    split-K 5.1    fp32 residual 5.9 (beyond the 2^-8 |want| of a bf16 output)
    No kernel of these is above the composition's 4 x margin, none needed a fix.  The kernels of gemm_x3.hip's row products, of
    gemm_wave.hip and the per-cloud products have no recorded figure yet: test_zz_measured_ratios prints them.

Mutants (one line each, on a scratch copy never committed, run on an MI355X; the tests each one fails):
1. the wgrad slice end rounded down to 16 rows: test_wgrad[f32-64x64xK-66-66-1] for K = 1, 2, 15, 17, 37, 255, 300 (K = 16 passes,
   as it must)
2. the KB = 4 LDS fold without its fourth wave: test_wgrad[f32-64x64x256-66-66-1], [f32-64x64x300-66-66-1],
   [f32-128x192x4113-130-194-1] and every test_wgrad_pair[*]
3. the reduce's tail step (`if (sl < SK)`) removed -- in wgrad_reduce_kernel: every test_wgrad[f32-64x64x*] (1 to 4 partials all
   take it); in wgrad_fold_body: every test_wgrad_pair[*], test_wgrad_fold_on_hand_made_partials[*],
   test_wgrad_fold_of_the_most_problems_in_one_launch, test_step_fold_with_both_kinds_of_entry
4. the column sum taken from tile tm == 1: test_wgrad[f32-64x64xK-66-66-1] for K = 1 ... 255 (one tile row: nothing writes the
   sum; with several tile rows every tm sums the same columns and the mutant is equivalent, 320x832 passes)
5. the x3 weight gradient without its lowest slice: every test_wgrad[f32-128x512xK-128-512-1]
6. the gemm_rows split boundary one k-block early in the second source: test_gemm_rows_f32[65x63-96nt+160nt-r-16],
   [63x65-160nt+96nn--8], test_gemm_rows_bf16[65x65-192nt+320nt-brc-16-*]
8. row / rows_per_cloud from the tile's first row: test_gemm_rows_f32[129x127-33nt+31nt-rc-16], [65x129-3nt+33nt-rc-4],
   [129x64-32nt-rcx-16], [64x64-255nt-brc-16], test_gemm_rows_bf16[65x63-64nt+65nt-rc-16-*], [129x64-33nt-rcx-16-*],
   [65x65-192nt+320nt-brc-16-*]
7. the x3 reduce without alpha, and 9. the panel kernel's row guard `<` replaced by `<=`: placed for test_gemm_x3_f32[63x128-512+512--ldc+4]
   (float4 fold, alpha 0.5) and [1130x4096-128--ldc+1] (M % 32 = 10); no recorded run.  Mutant 9 stays inside the buffer
   descriptor (row M starts past its last byte and reads as zeros) and its row is never stored: by reading it is equivalent.
None of the mutants reads or writes out of bounds.
"""
import ctypes
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _gemm_cases as gc
from hs_pose_amd._lib import HspDirsPending, HspWgradPending

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
NAN = float("nan")
INF = float("inf")
U = 2.0 ** -24
# The rule tests accept rule <= A <= 2 rule: torch.mm's blocking, and with it the composition's worst ratio, differs by CPU (13.1 and
# 18.4 seen for the weight gradients), and a constant has to hold on both.  Where the smaller figure is measured, A is one binade
# looser than "rounded up to a power of two"; never more.
A = 128.0                                  # the weight gradients: 4 x 18.4 = 73 (the project's 32 elsewhere does not hold here)
A_SUM = 16.0                               # the column sums: 4 x 3.5 = 13.8
A_ROWS = 64.0                              # the row products of gemm_rows.hip: 4 x 14.8 = 59
A_X3 = 128.0                               # the row products of gemm_x3.hip: 4 x 17.2 = 69
A_WAVE = 64.0                              # the wave kernel's cases: 4 x 9.5 = 38
A_SMALL = 64.0                             # the per-cloud products: 4 x 10.3 = 41
SENTINEL = -1.2345678e30
BAND = 4096                                # sentinel bytes behind a workspace
RATIOS = {}                                # what -> worst measured err / (2^-24 T), printed by the last test


def _L():
    from hs_pose_amd._lib import lib
    return lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- operands ---------------------------------------------------------------------------------------------------------------------

def _ranged(rows, cols, g):
    re = torch.randint(-12, 13, (rows, 1), generator=g).double()
    ce = torch.randint(-12, 13, (1, cols), generator=g).double()
    return (torch.randn(rows, cols, generator=g).double() * 2.0 ** re * 2.0 ** ce).float()


def _operands(K, M, N, seed, cancel, dtype=torch.float32):
    """A (K,M), B (K,N) as stored.  cancel: rows K/2 .. 2 (K/2) repeat the first half, permuted, A negated and perturbed"""
    g = torch.Generator().manual_seed(seed)
    a, b = _ranged(K, M, g), _ranged(K, N, g)
    h = K // 2
    if cancel and h:
        p = torch.randperm(h, generator=g)
        a[h:2 * h] = -a[:h][p] * (1 + 2.0 ** -10 * torch.randn(h, M, generator=g))
        b[h:2 * h] = b[:h][p]
    return a.to(dtype), b.to(dtype)


_REF = {}


def _reference(K, M, N, seed, cancel, dtype):
    """(A, B, want, T, want colsum, T colsum), computed once per data set and left unchanged"""
    key = (K, M, N, seed, cancel, dtype)
    if key not in _REF:
        a, b = _operands(K, M, N, seed, cancel, dtype)
        a64, b64 = a.double(), b.double()
        _REF[key] = (a, b, a64.t() @ b64, a64.abs().t() @ b64.abs(), b64.sum(0), b64.abs().sum(0))
    return _REF[key]


# ---- moats ------------------------------------------------------------------------------------------------------------------------

def _in_moat(t, ld, dev, al16=True):
    """t (rows, cols) -> a view with row pitch ld of a NaN parent on the device; al16: the view starts on 16 bytes, else 8 (4-byte
    elements) / 4 (2-byte elements) past such a boundary.  The parent is kept alive by the view."""
    rows, cols = t.shape
    assert ld >= cols
    lead = 64 + (0 if al16 else 2)
    parent = torch.full((lead + rows * ld + 64,), NAN, dtype=t.dtype, device=dev)
    v = parent.as_strided((rows, cols), (ld, 1), lead)
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == bool(al16)
    return v


class Out:
    """a NaN-prefilled (rows, cols) output with row pitch ld inside a parent of sentinels"""

    def __init__(self, rows, cols, ld, dev, dtype=torch.float32):
        self.parent = torch.full((32 + rows * ld + 32,), SENTINEL, dtype=dtype, device=dev)
        self.v = self.parent.as_strided((rows, cols), (ld, 1), 32)
        self.v.fill_(NAN)
        self.before = self._outside()

    def _outside(self):
        p = self.parent.clone()
        p.as_strided(self.v.shape, self.v.stride(), 32).zero_()
        return p.view(torch.int16)

    def intact(self):
        return torch.equal(self._outside(), self.before)


class Ws:
    """a workspace of exactly `nbytes` bytes with a sentinel band behind it"""

    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + BAND,), 0xA5, dtype=torch.uint8, device=dev)

    def intact(self):
        return bool((self.buf[self.nbytes:] == 0xA5).all())


def _takes(route, M, N, srcs, out, resid=None, bias=None, cb=None, xyz=None, alpha=1.0, rpc=0):
    """hsp_gemm_takes(route) for the call a test is about to make: srcs = [(A view, weight-side view, layout, K), ...], every
    operand where the entry point will read / write it"""
    from hs_pose_amd._lib import HspGemmCall
    (a1, b1, l1, K1), (a2, b2, l2, K2) = srcs if len(srcs) == 2 else (srcs[0], (None, None, 0, 0))
    ptr, ld = (lambda t: t.data_ptr() if t is not None else None), (lambda t: t.stride(0) if t is not None else 0)
    call = HspGemmCall(ptr(a1), ptr(b1), ptr(a2), ptr(b2), ptr(resid), ptr(out), M, N, K1, K2, l1, l2, 4, ld(a1), ld(b1), ld(a2), ld(b2),
                       ld(resid), ld(out), bias is not None, cb is not None, xyz is not None, False, alpha == 1.0, rpc, 0, 1)
    return _L().hsp_gemm_takes(ctypes.byref(call), route)


# ---- the bound --------------------------------------------------------------------------------------------------------------------

def _ratio(what, err, terms):
    ok = terms > 0
    r = (err[ok] / (U * terms[ok])).max().item() if ok.any() else 0.0
    RATIOS[what] = max(RATIOS.get(what, 0.0), r)
    return r


def _hold(got, want, terms, what, kind, A=A, rel=0.0):
    """|got - want| <= A 2^-24 T (+ rel |want|: 2^-8 for the one rounding of a bf16 output) element by element; a NaN left behind
    fails.  The reported ratio is that of the part of the error above rel |want|."""
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements (never written?)"
    err = (got - want).abs()
    print(f"  {what}: ratio {_ratio(kind, (err - rel * want.abs()).clamp_min(0), terms):.3f}")
    over = err - A * U * terms - rel * want.abs()
    i = int(over.argmax())
    assert over.flatten()[i] <= 0, (f"{what}: |err| {err.flatten()[i]:.3e} > {A} * 2^-24 * {terms.flatten()[i]:.3e} at "
                                    f"{np.unravel_index(i, over.shape)} (want {want.flatten()[i]:.6e})")


FORM_NAME = {gc.KB1: "wgrad fp32 MFMA, KB = 1", gc.KB4: "wgrad fp32 MFMA, KB = 4", gc.BF16: "wgrad bf16 MFMA", gc.X3: "wgrad x3"}


# ---- the entry points -------------------------------------------------------------------------------------------------------------

def _entry(c):
    return {"f32": "hsp_wgrad_f32", "bf16": "hsp_wgrad_bf16", "rbf16": "hsp_wgrad_ragged_bf16"}[c.entry]


def _dtype(c):
    return BF if "bf16" in c.entry else torch.float32


def _run_wgrad(c, a, b, colsum, dev, short=0, pend=None):
    """one call through the C ABI inside the moats -> (rc, C, colsum, workspace); pend (an HspWgradPending): through the case's
    ``_partial`` entry, which leaves the fold pending and describes it there"""
    L = _L()
    av, bv = _in_moat(a, c.lda, dev, c.al16), _in_moat(b, c.ldb, dev, c.al16)
    out = Out(c.M, c.N, c.N + 1, dev)
    cs = Out(1, c.N, c.N, dev) if colsum else None
    wsb = L.hsp_wgrad_workspace_bytes(c.M, c.N, c.K)
    ws = Ws(wsb, dev)
    entry, tail = _entry(c), (_stream(),)
    if pend is not None:                                                   # hsp_wgrad[_ragged]_partial_<rows>
        entry, tail = "_partial_".join(entry.rsplit("_", 1)), (ctypes.byref(pend), _stream())
    rc = getattr(L, entry)(_vp(av), c.lda, _vp(bv), c.ldb, c.M, c.N, c.K, _vp(out.v), c.N + 1, _vp(cs.v if cs else None),
                           _vp(ws.buf), wsb - short, *tail)
    torch.cuda.synchronize()
    return rc, out, cs, ws


def _ids(c):
    return f"{c.entry}-{c.M}x{c.N}x{c.K}-{c.lda}-{c.ldb}-{c.al16}"


# ==== the rule that sets A ========================================================================================================

def _seed(c):
    return 7000 + c.M + 3 * c.N + 5 * c.K


def test_fp32_composition_sets_A():
    """A = 4 x the worst ratio of torch.mm in fp32 on every case and data set, rounded up to a power of two.  (Needs no GPU: run it by its
    node id on a machine without one; the module mark keeps it out of a `-m "not gpu"` run.)"""
    worst = {}
    for c in gc.WGRAD:
        for cancel in (False, True):
            a, b, want, T, wcs, Tcs = _reference(c.K, c.M, c.N, _seed(c), cancel, _dtype(c))
            got = torch.mm(a.float().t().contiguous(), b.float())
            r = _ratio("composition C", (got.double() - want).abs(), T)
            rc = _ratio("composition colsum", (b.float().sum(0).double() - wcs).abs(), Tcs)
            assert r <= A and rc <= A_SUM, f"{c}: the composition itself is outside the bound ({r:.2f}, {rc:.2f})"
            worst["C"] = max(worst.get("C", 0), r)
            worst["colsum"] = max(worst.get("colsum", 0), rc)
            if cancel and c.K >= 64 and c.K % 2 == 0:                     # (an odd K leaves one row without its negative)
                assert (want.abs() <= 2.0 ** -5 * T).float().mean() > 0.9, f"{c}: the cancelling data set does not cancel"
    print("  composition ratios:", {k: round(v, 3) for k, v in worst.items()})
    for k, a in (("C", A), ("colsum", A_SUM)):                             # (torch.mm's blocking differs by CPU: 13.1 ... 18.4 seen)
        rule = 2.0 ** np.ceil(np.log2(4 * worst[k]))
        assert rule <= a <= 2 * rule, f"{k}: the composition's worst ratio {worst[k]:.3f} asks for A = {rule}"


# ==== weight gradients ============================================================================================================

@pytest.mark.parametrize("c", gc.WGRAD, ids=_ids)
def test_wgrad(dev, c):
    form, sk, ks, parts = gc.check_wgrad_plan(_L(), c)
    for cancel in (False, True):
        a, b, want, T, wcs, Tcs = _reference(c.K, c.M, c.N, _seed(c), cancel, _dtype(c))
        first = None
        for colsum in (True, False, True):                                # (the third call: the fixed-order fold gives the same bits)
            rc, out, cs, ws = _run_wgrad(c, a, b, colsum, dev)
            what = f"{_ids(c)} {'cancel' if cancel else 'range'} colsum={colsum}"
            assert rc == 0, f"{what}: rc {rc}"
            assert out.intact() and ws.intact() and (cs is None or cs.intact()), f"{what}: a write outside the output or past the workspace"
            if first is not None and colsum:
                assert torch.equal(out.v, first[0]) and torch.equal(cs.v, first[1]), f"{what}: two calls differ"
                continue
            _hold(out.v, want, T, what, FORM_NAME[form])
            if colsum:
                _hold(cs.v[0], wcs, Tcs, what + " colsum", FORM_NAME[form] + " colsum", A_SUM)
                first = (out.v.clone(), cs.v.clone())
                _partial_then_fold_gives(first, c, a, b, parts, dev, what)


def _partial_then_fold_gives(first, c, a, b, parts, dev, what):
    """the case's ``_partial`` entry, then its pending fold through hsp_wgrad_fold and, in a second run, through hsp_step_fold: the
    bits of the fold-now call (``first``), from the plan's count of partial sums, inside the moats"""
    L = _L()
    for fold in ("hsp_wgrad_fold", "hsp_step_fold"):
        pend = HspWgradPending()
        rc, out, cs, ws = _run_wgrad(c, a, b, True, dev, pend=pend)
        assert rc == 0, f"{what}: the partial entry's rc {rc}"
        assert pend.nparts == parts, f"{what}: {pend.nparts} partial sums pending, the plan says {parts}"
        p = ctypes.byref(pend)
        rc = L.hsp_wgrad_fold(p, 1, _stream()) if fold == "hsp_wgrad_fold" else L.hsp_step_fold(p, 1, None, 0, _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{what}: {fold} rc {rc}"
        assert torch.equal(out.v, first[0]) and torch.equal(cs.v, first[1]), f"{what}: partial + {fold} differs from the fold-now call"
        assert out.intact() and cs.intact() and ws.intact(), f"{what}: partial + {fold} wrote outside the output or past the workspace"


@pytest.mark.parametrize("c", gc.WGRAD_DECLINED, ids=_ids)
def test_wgrad_declines_what_its_plan_declines(dev, c):
    assert gc.wgrad_plan(_L(), c)[0] == -2
    a, b = _operands(c.K, c.M, c.N, 1, False, _dtype(c))
    rc, out, cs, ws = _run_wgrad(c, a, b, True, dev)
    assert rc == -2 and out.intact() and cs.intact() and ws.intact()
    assert torch.isnan(out.v).all() and torch.isnan(cs.v).all() and bool((ws.buf == 0xA5).all()), "a declined call wrote"


def test_wgrad_workspace_one_byte_short_is_declined(dev):
    for c in (gc.WGRAD[7], next(c for c in gc.WGRAD if c.form == gc.X3 and c.K == 1000 and c.M == 64)):
        a, b = _operands(c.K, c.M, c.N, 1, False, _dtype(c))
        rc, out, cs, ws = _run_wgrad(c, a, b, True, dev, short=1)
        assert rc == -3 and out.intact() and cs.intact() and ws.intact()
        assert torch.isnan(out.v).all() and torch.isnan(cs.v).all() and bool((ws.buf == 0xA5).all()), "a declined call wrote"


NONFINITE = [next(c for c in gc.WGRAD if c.form == f and c.entry == e and c.K == K and c.M == M)
             for f, e, K, M in ((gc.KB1, "f32", 255, 64), (gc.KB4, "f32", 300, 64), (gc.KB4, "f32", 4113, 128), (gc.X3, "f32", 257, 128),
                                (gc.X3, "f32", 257, 129), (gc.X3, "f32", 257, 771), (gc.BF16, "bf16", 257, 128),
                                (gc.KB4, "bf16", 257, 64), (gc.BF16, "rbf16", 257, 129), (gc.BF16, "rbf16", 257, 1286))]


@pytest.mark.parametrize("edge", [False, True], ids=["inside", "last-rows"])
@pytest.mark.parametrize("c", NONFINITE, ids=_ids)
def test_wgrad_nonfinite_is_confined(dev, c, edge):
    """one NaN and one Inf in A, one -Inf in B: C is non-finite in rows m1, m2 and column n3 and nowhere else -- `edge` puts them
    into the last valid K rows, next to the zero-filled tail of the last slice, and into the last valid row / column of C, next to
    the pad columns of a ragged M"""
    gc.check_wgrad_plan(_L(), c)
    a, b = _operands(c.K, c.M, c.N, _seed(c) + 1, False, _dtype(c))
    a, b = a.clone(), b.clone()
    K, M, N = c.K, c.M, c.N
    (k1, m1), (k2, m2), (k3, n3) = ((K - 1, M - 1), (K - 2, 0), (K - 1, N - 1)) if edge else ((K // 3, M // 2), (K // 2, 5), (2, 70 % N))
    a[k1, m1], a[k2, m2], b[k3, n3] = NAN, INF, -INF
    a64, b64 = a.double(), b.double()
    want = a64.t() @ b64
    bad = torch.zeros(M, N, dtype=torch.bool)
    bad[m1, :] = True
    bad[m2, :] = True
    bad[:, n3] = True
    assert torch.equal(~torch.isfinite(want), bad)
    fin = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))          # noqa: E731
    T = fin(a64).abs().t() @ fin(b64).abs()
    rc, out, cs, ws = _run_wgrad(c, a, b, True, dev)
    assert rc == 0 and out.intact() and cs.intact() and ws.intact()
    got = out.v.cpu().double()
    assert torch.equal(~torch.isfinite(got), bad), f"non-finite at {(~torch.isfinite(got) ^ bad).nonzero()[:8].tolist()} against the reference"
    if c.form != gc.X3:                                                      # (the x3 split turns Inf into Inf and NaN slices)
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(got[torch.isinf(want)], want[torch.isinf(want)])
    err = torch.where(bad, torch.zeros_like(got), (got - torch.where(bad, torch.zeros_like(want), want)).abs())
    assert (err <= A * U * T).all(), f"a finite element is outside the bound: {(err - A * U * T).max().item():.3e}"
    gcs = cs.v[0].cpu().double()
    csbad = torch.zeros(N, dtype=torch.bool)
    csbad[n3] = True
    assert torch.equal(~torch.isfinite(gcs), csbad) and (c.form == gc.X3 or gcs[n3] == -INF)
    e2 = torch.where(csbad, torch.zeros_like(gcs), (gcs - fin(b64).sum(0)).abs())
    assert (e2 <= A_SUM * U * fin(b64).abs().sum(0)).all()


# ==== the pair launch =============================================================================================================

def _rider_shape():
    """the smallest (B, N, C) the per-cloud column sum admits, by its own query"""
    L = _L()
    for C in range(1, 513):                                                 # smallest C first, then the fewest points, then clouds
        for N in range(1, 9):
            for B in range(1, 3):
                if L.hsp_colsum_cloud_ok(B, N, C, 0):
                    return B, N, C
    raise AssertionError("no shape admitted")


@pytest.mark.parametrize("rider", [False, True], ids=["pair", "pair+colsum"])
@pytest.mark.parametrize("p", gc.PAIRS, ids=lambda p: "-".join(str(v) for v in p[:6]))
def test_wgrad_pair(dev, p, rider):
    L = _L()
    M0, N0, K0, M1, N1, K1, one, shrunk = p
    plan = gc.check_pair_plan(L, p)
    prob, args = [], []
    for i, (M, N, K) in enumerate(((M0, N0, K0), (M1, N1, K1))):
        a, b, want, T, _, _ = _reference(K, M, N, 8000 + i + K, bool(i), torch.float32)
        av, bv = _in_moat(a, M + 2, dev), _in_moat(b, N + 2, dev)
        out = Out(M, N, N + 1, dev)
        ws = Ws(L.hsp_wgrad_workspace_bytes(M, N, K), dev)
        prob.append((av, bv, out, ws, want, T))
        args += [_vp(av), M + 2, _vp(bv), N + 2, M, N, K, _vp(out.v), N + 1, _vp(ws.buf), ws.nbytes]
    pend = (HspWgradPending * 2)()
    if rider:
        B, Np, C = _rider_shape()
        x = _ranged(B * Np, C, torch.Generator().manual_seed(5)).view(B, Np, C)
        xv = _in_moat(x.view(B * Np, C), C, dev)
        ro = Out(B, C, C, dev)
        rc = L.hsp_wgrad_partial_pair_colsum_f32(*args, pend, _vp(xv), B, Np, C, _vp(ro.v), _stream())
        torch.cuda.synchronize()
        if not one:
            assert rc == -2 and torch.isnan(ro.v).all() and all(torch.isnan(q[2].v).all() and bool((q[3].buf == 0xA5).all()) for q in prob)
            return
    else:
        rc = L.hsp_wgrad_partial_pair_f32(*args, pend, _stream())
    assert rc == 0
    if one:
        assert (pend[0].nparts, pend[1].nparts) == (plan[0] // 4, plan[2] // 4)
    assert L.hsp_wgrad_fold(pend, 2, _stream()) == 0
    torch.cuda.synchronize()
    for i, (av, bv, out, ws, want, T) in enumerate(prob):
        assert out.intact() and ws.intact(), "a write outside the output or past the workspace"
        form = gc.KB4 if one else (ctypes.c_int * 4)()
        if not one:
            M, N, K = p[3 * i:3 * i + 3]
            assert L.hsp_wgrad_plan(M, N, K, 4, 1, M + 2, N + 2, 0, form) == 0
            form = form[0]
        _hold(out.v, want, T, f"pair problem {i}", "wgrad pair launch" if one else FORM_NAME[form])
    if rider:
        assert ro.intact()
        _hold(ro.v, x.double().sum(1), x.double().abs().sum(1), "rider", "pair launch's column-sum rider", A_SUM)


# ==== the folds, on hand-made partials ============================================================================================

def _fold32(parts):
    """the documented order of wgrad_fold_body in fp32 on the CPU; parts (S, ...)"""
    S = parts.shape[0]
    red = []
    for g in range(4):
        s, s2, sl = torch.zeros_like(parts[0]), torch.zeros_like(parts[0]), g
        while sl + 4 < S:
            s, s2, sl = s + parts[sl], s2 + parts[sl + 4], sl + 8
        if sl < S:
            s = s + parts[sl]
        red.append(s + s2)
    return ((red[0] + red[1]) + red[2]) + red[3]


NPARTS = (1, 2, 3, 4, 5, 8, 9, 12, 13)


def _fold_problem(nparts, M, N, colsum, seed, dev):
    g = torch.Generator().manual_seed(seed)
    part = _ranged(nparts * M, N, g).view(nparts, M, N)
    csp = _ranged(nparts, N, g)
    buf = torch.cat([part.flatten(), csp.flatten()]).to(dev)               # the workspace layout: partials, then their column sums
    out, cs = Out(M, N, N + 1, dev), (Out(1, N, N, dev) if colsum else None)
    pd = HspWgradPending(buf.data_ptr(), buf.data_ptr() + 4 * nparts * M * N, out.v.data_ptr(), cs.v.data_ptr() if cs else 0, nparts, M, N, N + 1)
    return pd, buf, out, cs, _fold32(part), _fold32(csp)


def _check_folded(probs, what):
    for pd, buf, out, cs, want, wcs in probs:
        assert out.intact() and (cs is None or cs.intact()), f"{what}: a write outside the output"
        assert torch.equal(out.v.cpu(), want), f"{what}: nparts {pd.nparts}, {pd.M} x {pd.N}: not the fixed order's bits"
        if cs is not None:
            assert torch.equal(cs.v[0].cpu(), wcs), f"{what}: nparts {pd.nparts}: column sums are not the fixed order's bits"


@pytest.mark.parametrize("N", [4, 68])
@pytest.mark.parametrize("colsum", [False, True])
def test_wgrad_fold_on_hand_made_partials(dev, N, colsum):
    L = _L()
    probs = [_fold_problem(s, 3, N, colsum, 100 * N + s, dev) for s in NPARTS]
    for n in (1, 2):                                                        # one and two problems per launch, every slice count
        done = []
        for i in range(0, len(probs) - n + 1, n):
            for q in probs[i:i + n]:
                q[2].v.fill_(NAN)
            arr = (HspWgradPending * n)(*[q[0] for q in probs[i:i + n]])
            assert L.hsp_wgrad_fold(arr, n, _stream()) == 0
            done += probs[i:i + n]
        torch.cuda.synchronize()
        _check_folded(done, f"hsp_wgrad_fold, {n} per launch")


def test_wgrad_fold_of_the_most_problems_in_one_launch(dev):
    L = _L()
    n = gc.FOLD_MAX_WGRAD
    probs = [_fold_problem(NPARTS[i % len(NPARTS)], 3, (4, 68)[i % 2], i % 3 != 0, 300 + i, dev) for i in range(n)]
    arr = (HspWgradPending * n)(*[q[0] for q in probs])
    assert L.hsp_wgrad_fold(arr, n + 1, _stream()) == -1
    assert L.hsp_wgrad_fold(arr, n, _stream()) == 0
    torch.cuda.synchronize()
    _check_folded(probs, "hsp_wgrad_fold of HSP_FOLD_MAX_WGRAD")


def _dirs_fold64(part, dirs):
    """the direction fold in fp64: gD = (g - h (h . g)) / n, g = sum of the partials, n = ||D||, h = D / n -> (want, T), T the sum
    of the absolute terms (|g_d| + |h_d| sum_e |h_e| |g_e|) / n with |g| = sum of |partials|"""
    g, ga, D = part.double().sum(0), part.double().abs().sum(0), dirs.double()
    n = D.norm(dim=0)
    h = D / n
    return (g - h * (h * g).sum(0)) / n, (ga + h.abs() * (h.abs() * ga).sum(0)) / n


def test_step_fold_with_both_kinds_of_entry(dev):
    """the parameter-gradient entries bit for bit, as in the stand-alone fold; the direction entries against fp64 (see below)"""
    L = _L()
    probs = [_fold_problem(s, 3, N, cs, 500 + s + N, dev) for s, N, cs in ((1, 4, True), (5, 68, False), (13, 68, True), (8, 4, False))]
    dprobs = []
    for s, SC in ((1, 5), (17, 64), (40, 130)):
        g = torch.Generator().manual_seed(600 + s)
        part, dirs = _ranged(s * 3, SC, g).view(s, 3, SC), torch.randn(3, SC, generator=g)
        pb, db, out = part.to(dev), dirs.to(dev), Out(3, SC, SC, dev)
        dprobs.append((HspDirsPending(pb.data_ptr(), db.data_ptr(), out.v.data_ptr(), s, SC), pb, db, out) + _dirs_fold64(part, dirs))
    warr = (HspWgradPending * len(probs))(*[q[0] for q in probs])
    darr = (HspDirsPending * len(dprobs))(*[q[0] for q in dprobs])
    assert L.hsp_step_fold(warr, len(probs), darr, len(dprobs), _stream()) == 0
    torch.cuda.synchronize()
    _check_folded(probs, "hsp_step_fold")
    # The direction entries end in the Jacobian of F.normalize, whose operation order the header does not fix: they are held to
    # the fp64 formula.  First-order count of the roundings, each at most 2^-24 of a quantity T bounds: nparts - 1 in the fold;
    # n three multiplies, two adds and a root, a quotient per h, and h enters twice: 2 x 4; the dot product 5; the last
    # subtraction, multiplication and division 3 -> (nparts + 16) 2^-24 T.
    for pd, pb, db, out, want, T in dprobs:
        assert out.intact()
        _hold(out.v, want, T, f"hsp_step_fold: direction fold of {pd.nparts} partials", "step fold, direction entries", pd.nparts + 16.0)


# ==== row products: csrc/gemm_rows.hip ===========================================================================================
# C (M,N) = alpha * (A1 op(B1) + A2 op(B2)) + bias + resid + xyz3 . w3 + cloud_bias[row // rows_per_cloud]   (the header's order)

def _ld(K, align, es=4):
    """the smallest row pitch > K, in elements, whose bytes are a multiple of `align` and of nothing larger"""
    ld = K + 1
    while (ld * es) % align or (align < 16 and (ld * es) % (2 * align) == 0):
        ld += 1
    return ld


def _cancel_cols(a, b_nk, g):
    """forced cancellation along k: the second half of the k columns repeats the first, permuted, a negated and perturbed"""
    h = a.shape[1] // 2
    if h:
        p = torch.randperm(h, generator=g)
        a[:, h:2 * h] = -a[:, :h][:, p] * (1 + 2.0 ** -10 * torch.randn(a.shape[0], h, generator=g))
        b_nk[:, h:2 * h] = b_nk[:, :h][:, p]


# M, N, (K1, layout1), (K2, layout2) or None, epilogue "b" bias "r" resid "c" cloud bias "x" xyz3, rows per cloud, alpha, align,
# plan (tile edge, staging mode, splits); layout 0 = "nt" (N,K), 1 = "nn" (K,N)
R = namedtuple("R", "M N s1 s2 epi rpc alpha align plan")
ROWS = [
    R(1, 64, (1, 0), None, "", 0, 1.0, 16, (64, 1, 1)),
    R(63, 63, (3, 0), None, "b", 0, 1.0, 16, (64, 1, 1)),
    R(64, 64, (31, 1), None, "", 0, 1.0, 16, (64, 1, 1)),
    R(65, 65, (32, 0), None, "r", 0, 1.0, 8, (64, 2, 1)),                  # 8-byte rows
    R(65, 65, (33, 1), None, "br", 0, 0.5, 4, (64, 0, 1)),                 # 4-byte rows, "nn"
    R(129, 127, (33, 0), (31, 0), "rc", 50, 1.0, 16, (64, 1, 1)),          # a 64-row tile spans clouds of 50 rows, the last cloud 29
    R(65, 129, (3, 0), (33, 0), "rc", 25, 1.0, 4, (64, 0, 1)),             # three clouds in one tile, the last one 15 rows
    R(129, 128, (32, 1), (33, 0), "", 0, 1.0, 8, (64, 2, 1)),              # "nn" + "nt"
    R(64, 65, (6, 0), (34, 1), "b", 0, 1.0, 8, (64, 2, 1)),                # "nt" + "nn": issued with the sources swapped
    R(129, 64, (32, 0), None, "rcx", 43, 1.0, 16, (64, 1, 1)),             # the K = 3 rider of the epilogue
    # split-K: few tiles, >= 8 k-blocks of 32
    R(64, 64, (256, 0), None, "", 0, 1.0, 16, (64, 1, 2)),                 # the first shape that splits
    R(64, 64, (255, 0), None, "brc", 20, 2.0, 16, (64, 1, 2)),             # a ragged last block, the whole epilogue in the fold
    R(65, 63, (96, 0), (160, 0), "r", 0, 1.0, 16, (64, 1, 2)),             # the boundary (block 4) inside the second source
    R(63, 65, (160, 0), (96, 1), "", 0, 1.0, 8, (64, 2, 2)),               # swapped by the dispatch: the boundary is in its second source
    R(129, 129, (1025, 1), None, "b", 0, 1.0, 4, (64, 0, 7)),              # 33 blocks in 7 splits of 5, the last one 3
    R(64, 64, (224, 0), None, "", 0, 1.0, 16, (64, 1, 1)),                 # 7 blocks: one short of splitting
]
ROWS_BF16 = [
    R(1, 64, (1, 0), None, "", 0, 1.0, 16, (64, 1, 1)),
    R(63, 65, (63, 0), None, "b", 0, 1.0, 16, (64, 1, 1)),
    R(65, 63, (64, 0), (65, 0), "rc", 25, 1.0, 16, (64, 1, 1)),
    R(129, 64, (33, 0), None, "rcx", 50, 0.5, 16, (64, 1, 1)),
    R(64, 64, (512, 0), None, "", 0, 1.0, 16, (64, 1, 2)),                 # 8 blocks of 64: the first shape that splits
    R(65, 65, (192, 0), (320, 0), "brc", 30, 1.0, 16, (64, 1, 2)),         # the boundary (block 4) inside the second source
]


def _rows_data(c, seed, cancel, dtype):
    g = torch.Generator().manual_seed(seed)
    d = SimpleNamespace(src=[])
    for s in (c.s1, c.s2):
        if s is None:
            continue
        K, lay = s
        a, b = _ranged(c.M, K, g), _ranged(c.N, K, g)                       # b as (N, K)
        if cancel:
            _cancel_cols(a, b, g)
        d.src.append((a.to(dtype), (b.t().contiguous() if lay else b).to(dtype), lay, K))
    d.bias = _ranged(1, c.N, g)[0] if "b" in c.epi else None
    d.resid = _ranged(c.M, c.N, g) if "r" in c.epi else None
    d.cb = _ranged(-(-c.M // c.rpc), c.N, g) if "c" in c.epi else None
    d.xyz, d.w3 = (_ranged(c.M, 3, g), _ranged(c.N, 3, g)) if "x" in c.epi else (None, None)
    return d


def _rows_ref(c, d, dt=F64):
    """the product and the epilogue in the header's order -> (want, T); dt = float32: the torch composition"""
    y, T = 0, 0
    for a, b, lay, K in d.src:
        bb = b.to(dt) if lay else b.to(dt).t()
        y = y + a.to(dt) @ bb
        T = T + a.double().abs() @ (b.double().abs() if lay else b.double().abs().t())
    y, T = c.alpha * y, abs(c.alpha) * T
    for add in (d.bias, d.resid):
        if add is not None:
            y, T = y + add.to(dt), T + add.double().abs()
    if d.xyz is not None:
        y, T = y + d.xyz.to(dt) @ d.w3.to(dt).t(), T + d.xyz.double().abs() @ d.w3.double().abs().t()
    if d.cb is not None:
        rows = torch.arange(c.M) // c.rpc
        y, T = y + d.cb.to(dt)[rows], T + d.cb.double().abs()[rows]
    return y, T


_ROWS_REF = {}


def _rows_case(c, cancel, dtype=torch.float32, resid_f32=False):
    key = (c, cancel, dtype, resid_f32)
    if key not in _ROWS_REF:
        d = _rows_data(c, 9000 + c.M + 3 * c.N + 7 * c.s1[0] + (11 * c.s2[0] if c.s2 else 0), cancel, dtype)
        if d.resid is not None and dtype == BF and not resid_f32:
            d.resid = d.resid.to(BF)
        _ROWS_REF[key] = (d,) + _rows_ref(c, d)
    return _ROWS_REF[key]


def rows_plan(c, es):
    out = (ctypes.c_int * 4)()
    rc = _L().hsp_gemm_rows_plan(c.M, c.N, c.s1[0], c.s2[0] if c.s2 else 0, es, c.align, out)
    return rc, tuple(out[:3])


def _run_rows(c, d, dev, entry="f32", c_f32=True, short=0, no_ws=False, ldc_pad=1):
    """one call through the C ABI inside the moats -> (rc, C, workspace)"""
    L = _L()
    es = 4 if entry == "f32" else 2
    ops_ = []
    for a, b, lay, K in d.src:
        av = _in_moat(a, _ld(K, c.align, es), dev)
        bv = _in_moat(b, _ld(b.shape[1], c.align, es), dev)
        ops_ += [(av, av.stride(0), bv, bv.stride(0), lay, K)]
    if len(ops_) == 1:
        ops_.append((None, 0, None, 0, 0, 0))
    ldc = c.N + ldc_pad
    out = Out(c.M, c.N, ldc, dev, torch.float32 if c_f32 else BF)
    resid = _in_moat(d.resid, c.N + 3, dev) if d.resid is not None else None
    bias = _in_moat(d.bias[None], c.N, dev) if d.bias is not None else None
    cb = _in_moat(d.cb, c.N, dev) if d.cb is not None else None
    xyz = _in_moat(d.xyz, 3, dev) if d.xyz is not None else None
    w3 = _in_moat(d.w3, 3, dev) if d.w3 is not None else None
    wsb = L.hsp_gemm_rows_workspace_bytes(c.M, c.N, c.s1[0], c.s2[0] if c.s2 else 0, es)
    ws = Ws(wsb, dev)
    wsp, wsn = (_vp(None), 0) if no_ws else (_vp(ws.buf), wsb - short)
    (a1, la1, b1, lb1, l1, K1), (a2, la2, b2, lb2, l2, K2) = ops_
    if entry == "f32":
        rc = L.hsp_gemm_rows_f32(_vp(a1), la1, _vp(b1), lb1, l1, K1, _vp(a2), la2, _vp(b2), lb2, l2, K2, c.M, c.N, _vp(bias), _vp(resid),
                                 c.N + 3, _vp(cb), c.rpc, c.alpha, _vp(xyz), _vp(w3), _vp(out.v), ldc, wsp, wsn, _stream())
    elif entry == "bf16":
        rc = L.hsp_gemm_rows_bf16(_vp(a1), la1, _vp(b1), lb1, K1, _vp(a2), la2, _vp(b2), lb2, K2, c.M, c.N, _vp(bias), _vp(resid), c.N + 3,
                                  _vp(cb), c.rpc, c.alpha, _vp(xyz), _vp(w3), _vp(out.v), ldc, int(c_f32), wsp, wsn, _stream())
    else:
        rc = L.hsp_gemm_rows_acc_bf16(_vp(a1), la1, _vp(b1), lb1, K1, _vp(a2), la2, _vp(b2), lb2, K2, c.M, c.N, _vp(resid), c.N + 3,
                                      _vp(out.v), ldc, int(c_f32), wsp, wsn, _stream())
    torch.cuda.synchronize()
    return rc, out, ws


def _rid(c):
    return f"{c.M}x{c.N}-{c.s1[0]}{'nn' if c.s1[1] else 'nt'}" + (f"+{c.s2[0]}{'nn' if c.s2[1] else 'nt'}" if c.s2 else "") + f"-{c.epi}-{c.align}"


def test_fp32_composition_sets_A_rows():
    """the same rule for the row products.  (Needs no GPU.)"""
    worst = 0.0
    for c in ROWS + ROWS_BF16:
        for cancel in (False, True):
            d, want, T = _rows_case(c, cancel, BF if c in ROWS_BF16 and c not in ROWS else torch.float32)
            got, _ = _rows_ref(c, d, torch.float32)
            r = _ratio("composition rows", (got.double() - want).abs(), T)
            assert r <= A_ROWS, f"{c}: the composition itself is outside the bound ({r:.2f})"
            worst = max(worst, r)
    print(f"  composition ratio, rows: {worst:.3f}")
    rule = 2.0 ** np.ceil(np.log2(4 * worst))
    assert rule <= A_ROWS <= 2 * rule, f"the composition's worst ratio {worst:.3f} asks for A = {rule}"


@pytest.mark.parametrize("c", ROWS, ids=_rid)
def test_gemm_rows_f32(dev, c):
    assert rows_plan(c, 4) == (0, c.plan)
    ns = c.plan[2]
    for cancel in (False, True):
        d, want, T = _rows_case(c, cancel)
        kind = "gemm_rows fp32" + (", split-K" if ns > 1 else "")
        rc, out, ws = _run_rows(c, d, dev)
        what = f"{_rid(c)} {'cancel' if cancel else 'range'}"
        assert rc == 0 and out.intact() and ws.intact(), f"{what}: rc {rc}, or a write outside the output / past the workspace"
        _hold(out.v, want, T, what, kind, A_ROWS)
        if ns > 1:
            again = _run_rows(c, d, dev)[1]
            assert torch.equal(again.v, out.v), f"{what}: the fixed-order fold gave other bits on a second call"
            # a workspace one byte short, or none: the unsplit product, inside the same bound
            for kw in ({"short": 1}, {"no_ws": True}):
                rc, o2, w2 = _run_rows(c, d, dev, **kw)
                assert rc == 0 and o2.intact() and bool((w2.buf == 0xA5).all()), f"{what} {kw}: the workspace was written"
                _hold(o2.v, want, T, f"{what} {kw}", "gemm_rows fp32", A_ROWS)


@pytest.mark.parametrize("c_f32", [False, True], ids=["C-bf16", "C-fp32"])
@pytest.mark.parametrize("c", ROWS_BF16, ids=_rid)
def test_gemm_rows_bf16(dev, c, c_f32):
    assert rows_plan(c, 2) == (0, c.plan)
    for cancel in (False, True):
        d, want, T = _rows_case(c, cancel, BF)
        for pad in (1, 2):                                                  # (a bf16 C with even N and pitch is stored in column pairs)
            rc, out, ws = _run_rows(c, d, dev, "bf16", c_f32, ldc_pad=pad)
            what = f"{_rid(c)} {'cancel' if cancel else 'range'} ldc=N+{pad}"
            assert rc == 0 and out.intact() and ws.intact(), f"{what}: rc {rc}, or a write outside the output / past the workspace"
            _hold(out.v, want, T, what, "gemm_rows bf16" + (", split-K" if c.plan[2] > 1 else ""), A_ROWS, 0.0 if c_f32 else 2.0 ** -8)
        if c.plan[2] > 1:
            rc, o2, w2 = _run_rows(c, d, dev, "bf16", c_f32, short=1)
            assert rc == 0 and o2.intact() and bool((w2.buf == 0xA5).all())
            _hold(o2.v, want, T, what + " short", "gemm_rows bf16", A_ROWS, 0.0 if c_f32 else 2.0 ** -8)


@pytest.mark.parametrize("c_f32", [False, True], ids=["C-bf16", "C-fp32"])
@pytest.mark.parametrize("c", [c for c in ROWS_BF16 if "r" in c.epi], ids=_rid)
def test_gemm_rows_acc_bf16(dev, c, c_f32):
    """bf16 operands, an fp32 residual, nothing else in the epilogue"""
    c = c._replace(epi="r", alpha=1.0)
    assert rows_plan(c, 2) == (0, c.plan)
    for cancel in (False, True):
        d, want, T = _rows_case(c, cancel, BF, True)
        rc, out, ws = _run_rows(c, d, dev, "acc", c_f32)
        assert rc == 0 and out.intact() and ws.intact()
        _hold(out.v, want, T, f"{_rid(c)} acc", "gemm_rows bf16, fp32 residual", A_ROWS, 0.0 if c_f32 else 2.0 ** -8)


@pytest.mark.parametrize("edge", [False, True], ids=["inside", "last-rows"])
@pytest.mark.parametrize("entry,c", [("f32", ROWS[5]), ("f32", ROWS[12]), ("f32", ROWS[14]), ("bf16", ROWS_BF16[2]), ("bf16", ROWS_BF16[5])],
                         ids=lambda v: v if isinstance(v, str) else _rid(v))
def test_gemm_rows_nonfinite_is_confined(dev, entry, c, edge):
    """a NaN in one row of A1, an Inf in another, a -Inf in one row of the last source's B: C is non-finite in those two rows and
    that column and nowhere else -- `edge`: the last valid row / column / k, next to the clamped rows and the zero-filled tail"""
    dtype = torch.float32 if entry == "f32" else BF
    d0, _, _ = _rows_case(c, False, dtype)
    d = SimpleNamespace(**vars(d0))
    d.src = [(a.clone(), b.clone(), lay, K) for a, b, lay, K in d0.src]
    M, N = c.M, c.N
    K1, Kl = d.src[0][3], d.src[-1][3]
    (r1, k1), (r2, k2), (n3, k3) = ((M - 1, K1 - 1), (M - 2, 0), (N - 1, Kl - 1)) if edge else ((M // 3, K1 // 2), (M // 2, 1), (N // 2, Kl // 3))
    d.src[0][0][r1, k1] = NAN
    d.src[0][0][r2, k2] = INF
    bl, lay = d.src[-1][1], d.src[-1][2]
    if lay:
        bl[k3, n3] = -INF
    else:
        bl[n3, k3] = -INF
    want, _ = _rows_ref(c, d)
    bad = torch.zeros(M, N, dtype=torch.bool)
    bad[r1, :] = True
    bad[r2, :] = True
    bad[:, n3] = True
    assert torch.equal(~torch.isfinite(want), bad)
    fin = SimpleNamespace(**vars(d))
    fin.src = [(torch.nan_to_num(a.float(), 0.0, 0.0, 0.0).to(dtype), torch.nan_to_num(b.float(), 0.0, 0.0, 0.0).to(dtype), lay, K) for a, b, lay, K in d.src]
    wfin, T = _rows_ref(c, fin)
    rc, out, ws = _run_rows(c, d, dev, entry)
    assert rc == 0 and out.intact() and ws.intact()
    got = out.v.cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN elsewhere than the reference has it"
    assert torch.equal(got[torch.isinf(want)], want[torch.isinf(want)])
    err = torch.where(bad, torch.zeros_like(got), (got - wfin).abs())
    assert (err <= A_ROWS * U * T).all(), f"a finite element is outside the bound: {(err - A_ROWS * U * T).max().item():.3e}"


# ==== row products on the bf16 matrix cores from three-way splits: csrc/gemm_x3.hip ==============================================
# the contract of gemm_rows ("nt" weights, no xyz3 rider); the weight comes as three bf16 planes (N, ldp), columns K .. ceil32(K) zero

def _planes(w, dev):
    """w (N, K) fp32 -> (planes on the device inside a NaN moat, ldp, ps): x = hi + mid + lo by truncation, as hsp_split_params_x3
    writes them; row pitch ldp = ceil32(K) + 8 with the columns past ceil32(K) left NaN, 8 NaN elements between the planes"""
    N, K = w.shape
    kp = (K + 31) // 32 * 32
    ldp, lead = kp + 8, 64
    ps = N * ldp + 8
    trunc = lambda x: (x.view(torch.int32) & -65536).view(torch.float32)         # noqa: E731
    hi = trunc(w)
    r1 = w - hi
    mid = trunc(r1)
    lo = trunc(r1 - mid)
    buf = torch.full((lead + 3 * ps + 64,), NAN, dtype=BF)
    for p, x in enumerate((hi, mid, lo)):
        assert torch.equal(x.to(BF).float(), x) or not torch.isfinite(x).all()
        v = buf.as_strided((N, kp), (ldp, 1), lead + p * ps)
        v.zero_()
        v[:, :K] = x.to(BF)
    assert torch.equal(hi + mid + lo, w) or not torch.isfinite(w).all()
    d = buf.to(dev)
    return d, d.as_strided((N, kp), (ldp, 1), lead), ldp, ps


# plan: (panel kernel, tile height / 64, splits, fold path 4 = float4 | 1 = scalar | 0 = none)
X = namedtuple("X", "M N s1 s2 epi rpc alpha ldc_pad plan")
X3 = [
    X(1, 64, (993, 0), None, "", 0, 1.0, 4, (0, 1, 4, 4)),                 # admitted by its 32 k-blocks alone; one tile in 4 splits
    X(961, 1024, (1, 0), None, "b", 0, 1.0, 1, (0, 1, 1, 0)),              # admitted by its 128 tiles of 64 rows alone
    X(65, 1286, (1024, 0), None, "", 0, 1.0, 1, (0, 1, 4, 1)),             # the scalar fold: N % 4 = 2, M odd
    X(63, 128, (512, 0), (512, 0), "", 0, 0.5, 4, (0, 1, 4, 4)),           # the float4 fold with alpha; split 3 starts inside source 2
    X(129, 65, (993, 0), None, "b", 0, 2.0, 1, (0, 1, 1, 0)),              # any epilogue: unsplit
    X(129, 65, (500, 0), (530, 0), "rc", 25, 1.0, 1, (0, 1, 1, 0)),        # clouds shorter than the tile: the division path
    X(129, 130, (500, 0), (530, 0), "rc", 100, 0.5, 1, (0, 1, 1, 0)),      # two clouds in a tile: the boundary compare
    X(65, 64, (1000, 0), None, "r", 0, 1.0, 1, (0, 1, 1, 0)),              # residual alone: the accumulators start from it
    X(65, 127, (1000, 0), None, "c", 30, 1.0, 1, (0, 1, 1, 0)),            # per-cloud bias alone
    X(2041, 4096, (33, 0), None, "b", 0, 1.0, 1, (0, 2, 1, 0)),            # 512 tiles of 128 rows: the 128-row tile
    X(1130, 4096, (128, 0), None, "", 0, 0.5, 1, (1, 0, 1, 0)),            # the panel kernel's smallest fill (36 row tiles), M % 32 = 10
    X(1152, 4096, (128, 0), None, "b", 0, 1.0, 4, (1, 0, 1, 0)),           # whole row tiles, bias
    X(1120, 4096, (128, 0), None, "b", 0, 1.0, 1, (0, 1, 1, 0)),           # 35 row tiles fill 0.73 of three rounds: the tile kernel
]
X3_REFUSED = [(1, 64, 992, 0), (8128, 64, 992, 0), (960, 1024, 1, 0), (960, 1024, 480, 480), (100, 63, 2000, 0)]
# shapes hsp_gemm_x3_supported admits in calls the kernel has no form for: a residual alone with alpha != 1 (ops.gemm_own used to
# send it there) or with two sources, bias + residual
X3_REFUSED_CALLS = [X(65, 64, (1000, 0), None, "r", 0, 0.5, 1, None), X(63, 128, (512, 0), (512, 0), "r", 0, 1.0, 4, None),
                    X(129, 65, (993, 0), None, "br", 0, 1.0, 1, None)]


def x3_plan(c, ldc):
    out = (ctypes.c_int * 4)()
    epi = (1 if "b" in c.epi else 0) | (2 if "r" in c.epi else 0) | (4 if "c" in c.epi else 0)
    rc = _L().hsp_gemm_x3_plan(c.M, c.N, c.s1[0], c.s2[0] if c.s2 else 0, epi, ldc, out)
    return rc, tuple(out)


def _run_x3(c, d, dev, short=0):
    L = _L()
    srcs = []
    for a, w, lay, K in d.src:
        av = _in_moat(a, (K + 3) // 4 * 4 + 4, dev)
        buf, pv, ldp, ps = _planes(w, dev)
        srcs.append((av, av.stride(0), buf, pv, ldp, ps, K))
    if len(srcs) == 1:
        srcs.append((None, 0, None, None, 0, 0, 0))
    ldc = c.N + c.ldc_pad
    out = Out(c.M, c.N, ldc, dev)
    resid = _in_moat(d.resid, c.N + 3, dev) if d.resid is not None else None
    bias = _in_moat(d.bias[None], c.N, dev) if d.bias is not None else None
    cb = _in_moat(d.cb, c.N, dev) if d.cb is not None else None
    wsb = L.hsp_gemm_x3_workspace_bytes(c.M, c.N, c.s1[0], c.s2[0] if c.s2 else 0)
    ws = Ws(wsb, dev)
    (a1, la1, _, p1, lp1, ps1, K1), (a2, la2, _, p2, lp2, ps2, K2) = srcs
    out.takes = _takes(gc.X3R, c.M, c.N, [(a1, p1, 0, K1)] + ([(a2, p2, 0, K2)] if a2 is not None else []), out.v, resid, bias, cb,
                       alpha=c.alpha, rpc=c.rpc)
    rc = L.hsp_gemm_x3_f32(_vp(a1), la1, _vp(p1), lp1, ps1, K1, _vp(a2), la2, _vp(p2), lp2, ps2, K2, c.M, c.N, _vp(bias), _vp(resid),
                           c.N + 3, _vp(cb), c.rpc, c.alpha, _vp(out.v), ldc, _vp(ws.buf), wsb - short, _stream())
    torch.cuda.synchronize()
    return rc, out, ws


def _xid(c):
    return f"{c.M}x{c.N}-{c.s1[0]}" + (f"+{c.s2[0]}" if c.s2 else "") + f"-{c.epi}-ldc+{c.ldc_pad}"


def test_fp32_composition_sets_A_x3():
    """the same rule for the x3 row products.  (Needs no GPU.)"""
    worst = 0.0
    for c in X3:
        for cancel in (False, True):
            d, want, T = _rows_case(c, cancel)
            got, _ = _rows_ref(c, d, torch.float32)
            r = _ratio("composition x3 rows", (got.double() - want).abs(), T)
            assert r <= A_X3, f"{c}: the composition itself is outside the bound ({r:.2f})"
            worst = max(worst, r)
    print(f"  composition ratio, x3 rows: {worst:.3f}")
    rule = 2.0 ** np.ceil(np.log2(4 * worst))
    assert rule <= A_X3 <= 2 * rule, f"the composition's worst ratio {worst:.3f} asks for A = {rule}"


@pytest.mark.parametrize("c", X3, ids=_xid)
def test_gemm_x3_f32(dev, c):
    assert _L().hsp_gemm_x3_supported(c.M, c.N, c.s1[0], c.s2[0] if c.s2 else 0) == 1
    assert x3_plan(c, c.N + c.ldc_pad) == (0, c.plan)
    panel, wm, ns, path = c.plan
    kind = "gemm_x3 panel kernel" if panel else "gemm_x3 tile kernel" + (", split-K" if ns > 1 else "")
    for cancel in (False, True):
        d, want, T = _rows_case(c, cancel)
        what = f"{_xid(c)} {'cancel' if cancel else 'range'}"
        rc, out, ws = _run_x3(c, d, dev)
        assert out.takes == 1 and rc == 0, f"{what}: hsp_gemm_takes {out.takes}, the entry point {rc}"
        assert out.intact() and ws.intact(), f"{what}: a write outside the output / past the workspace"
        _hold(out.v, want, T, what, kind, A_X3)
        if ns > 1:
            assert torch.equal(_run_x3(c, d, dev)[1].v, out.v), f"{what}: the fixed-order fold gave other bits on a second call"
            rc, o2, w2 = _run_x3(c, d, dev, short=1)                       # a workspace too small: silently unsplit
            assert rc == 0 and o2.intact() and bool((w2.buf == 0xA5).all()), f"{what}: a too-small workspace was written"
            _hold(o2.v, want, T, what + " short workspace", "gemm_x3 tile kernel", A_X3)


def test_gemm_x3_refuses_below_both_clauses(dev):
    """the largest shapes hsp_gemm_x3_supported refuses on each clause (31 k-blocks; 127 / 120 tiles of 64 rows) and N < 64:
    HSP_ERR_UNSUPPORTED, nothing written"""
    L = _L()
    for M, N, K1, K2 in X3_REFUSED:
        assert L.hsp_gemm_x3_supported(M, N, K1, K2) == 0 and L.hsp_gemm_x3_workspace_bytes(M, N, K1, K2) == 0
        out = (ctypes.c_int * 4)()
        assert L.hsp_gemm_x3_plan(M, N, K1, K2, 0, N, out) == -2
        c = X(M, N, (K1, 0), (K2, 0) if K2 else None, "", 0, 1.0, 1, None)
        d = _rows_data(c, 1, False, torch.float32)
        rc, o, ws = _run_x3(c, d, dev)
        assert o.takes == 0 and rc == -2 and o.intact() and torch.isnan(o.v).all() and bool((ws.buf == 0xA5).all())
    for c in X3_REFUSED_CALLS:
        assert L.hsp_gemm_x3_supported(c.M, c.N, c.s1[0], c.s2[0] if c.s2 else 0) == 1
        rc, o, ws = _run_x3(c, _rows_data(c, 1, False, torch.float32), dev)
        assert o.takes == 0 and rc == -2 and o.intact() and torch.isnan(o.v).all() and bool((ws.buf == 0xA5).all()), _xid(c)


@pytest.mark.parametrize("edge", [False, True], ids=["inside", "last-rows"])
@pytest.mark.parametrize("c", [X3[3], X3[5], X3[10]], ids=_xid)
def test_gemm_x3_nonfinite_is_confined(dev, c, edge):
    """a NaN in one row of A1, an Inf in another, a -Inf in one row of the last weight: the x3 split turns an Inf into Inf and NaN
    slices, so C must be non-finite exactly in those two rows and that column, and finite and inside the bound elsewhere"""
    d0, _, _ = _rows_case(c, False)
    d = SimpleNamespace(**vars(d0))
    d.src = [(a.clone(), b.clone(), lay, K) for a, b, lay, K in d0.src]
    M, N = c.M, c.N
    K1, Kl = d.src[0][3], d.src[-1][3]
    (r1, k1), (r2, k2), (n3, k3) = ((M - 1, K1 - 1), (M - 2, 0), (N - 1, Kl - 1)) if edge else ((M // 3, K1 // 2), (M // 2, 1), (N // 2, Kl // 3))
    d.src[0][0][r1, k1] = NAN
    d.src[0][0][r2, k2] = INF
    d.src[-1][1][n3, k3] = -INF
    want, _ = _rows_ref(c, d)
    bad = torch.zeros(M, N, dtype=torch.bool)
    bad[r1, :] = True
    bad[r2, :] = True
    bad[:, n3] = True
    assert torch.equal(~torch.isfinite(want), bad)
    fin = SimpleNamespace(**vars(d))
    fin.src = [(torch.nan_to_num(a, 0.0, 0.0, 0.0), torch.nan_to_num(b, 0.0, 0.0, 0.0), lay, K) for a, b, lay, K in d.src]
    wfin, T = _rows_ref(c, fin)
    rc, out, ws = _run_x3(c, d, dev)
    assert rc == 0 and out.intact() and ws.intact()
    got = out.v.cpu().double()
    assert torch.equal(~torch.isfinite(got), bad), f"non-finite at {(~torch.isfinite(got) ^ bad).nonzero()[:8].tolist()} against the reference"
    err = torch.where(bad, torch.zeros_like(got), (got - wfin).abs())
    assert (err <= A_X3 * U * T).all(), f"a finite element is outside the bound: {(err - A_X3 * U * T).max().item():.3e}"


# ==== the per-cloud products: hsp_small_rows_f32, hsp_small_outer_f32, hsp_small_pair_f32 (csrc/gemm_x3.hip) ====================

# M, N, K, layout (0 "nt": W (N,K); 1 "nn": W (K,N)), alpha, rows on 16 bytes, the form: "mfma" (K % 128 == 0; "nt" needs aligned rows) | "lanes"
SMALL_ROWS = [
    (1, 16, 128, 0, 1.0, True, "mfma"), (2, 17, 128, 1, 0.5, False, "mfma"), (16, 33, 256, 0, 1.0, True, "mfma"),
    (64, 40, 512, 1, 2.0, True, "mfma"), (17, 16, 128, 1, 1.0, True, "mfma"), (64, 15, 2048, 0, 1.0, True, "mfma"),
    (1, 8, 1, 0, 1.0, True, "lanes"), (2, 9, 37, 0, 0.5, False, "lanes"), (16, 70, 100, 1, 1.0, False, "lanes"),
    (16, 65, 127, 0, 1.0, True, "lanes"), (2, 9, 128, 0, 1.0, False, "lanes"), (1, 130, 65, 1, 1.0, True, "lanes"),
]
# B, Ma, Nb, Cm of the moment rider (0 = none)
SMALL_OUTER = [(1, 3, 5, 0), (2, 64, 64, 4), (16, 33, 7, 0), (17, 5, 300, 100), (64, 128, 65, 0)]
# B, Ma, Nn, Nb, Cm
SMALL_PAIR = [(1, 128, 16, 5, 0), (2, 256, 17, 64, 4), (16, 128, 33, 33, 0), (64, 128, 40, 16, 100)]


def _small_rows_data(M, N, K, lay, cancel, seed):
    g = torch.Generator().manual_seed(seed)
    a, w = _ranged(M, K, g), _ranged(N, K, g)
    if cancel:
        _cancel_cols(a, w, g)
    return a, (w.t().contiguous() if lay else w)


def _small_rows_ref(a, w, lay, alpha, dt=F64):
    ww = w.to(dt) if lay else w.to(dt).t()
    return alpha * (a.to(dt) @ ww), abs(alpha) * (a.double().abs() @ (w.double().abs() if lay else w.double().abs().t()))


def _run_small_rows(a, w, lay, alpha, al, dev):
    M, K = a.shape
    N = w.shape[1] if lay else w.shape[0]
    pad = 4 if al else 1
    av = _in_moat(a, (K + 3) // 4 * 4 + pad, dev)
    wv = _in_moat(w, (w.shape[1] + 3) // 4 * 4 + pad, dev)
    out = Out(M, N, N + 1, dev)
    out.takes = _takes(gc.SMALL, M, N, [(av, wv, lay, K)], out.v, alpha=alpha)
    rc = _L().hsp_small_rows_f32(_vp(av), av.stride(0), _vp(wv), wv.stride(0), lay, M, N, K, alpha, _vp(out.v), N + 1, _stream())
    torch.cuda.synchronize()
    return rc, out


def _outer_data(B, Ma, Nb, Cm, cancel, seed):
    g = torch.Generator().manual_seed(seed)
    a, c = _ranged(B, Ma, g), _ranged(B, Nb, g)
    h = B // 2
    if cancel and h:
        p = torch.randperm(h, generator=g)
        a[h:2 * h] = -a[:h][p] * (1 + 2.0 ** -10 * torch.randn(h, Ma, generator=g))
        c[h:2 * h] = c[:h][p]
    mom = _ranged(B, 3 * Cm, g) if Cm else None
    return a, c, mom


def _gste_ref(mom, Cm, dt=F64):
    """gste (Cm, 3)[c][j] = sum_b mom[b][j * Cm + c]"""
    return mom.to(dt).sum(0).view(3, Cm).t(), mom.double().abs().sum(0).view(3, Cm).t()


def test_fp32_composition_sets_A_small():
    """the same rule for the per-cloud products.  (Needs no GPU.)"""
    worst = 0.0
    for i, (M, N, K, lay, alpha, al, form) in enumerate(SMALL_ROWS):
        for cancel in (False, True):
            a, w = _small_rows_data(M, N, K, lay, cancel, 300 + i)
            want, T = _small_rows_ref(a, w, lay, alpha)
            worst = max(worst, _ratio("composition small", (_small_rows_ref(a, w, lay, alpha, torch.float32)[0].double() - want).abs(), T))
    for i, (B, Ma, Nb, Cm) in enumerate(SMALL_OUTER):
        for cancel in (False, True):
            a, c, mom = _outer_data(B, Ma, Nb, Cm, cancel, 400 + i)
            want, T = a.double().t() @ c.double(), a.double().abs().t() @ c.double().abs()
            worst = max(worst, _ratio("composition small", (torch.mm(a.t().contiguous(), c).double() - want).abs(), T))
            if Cm:
                worst = max(worst, _ratio("composition small", (_gste_ref(mom, Cm, torch.float32)[0].double() - _gste_ref(mom, Cm)[0]).abs(),
                                          _gste_ref(mom, Cm)[1]))
    print(f"  composition ratio, small products: {worst:.3f}")
    rule = 2.0 ** np.ceil(np.log2(4 * worst))
    assert rule <= A_SMALL <= 2 * rule, f"the composition's worst ratio {worst:.3f} asks for A = {rule}"


@pytest.mark.parametrize("M,N,K,lay,alpha,al,form", SMALL_ROWS)
def test_small_rows(dev, M, N, K, lay, alpha, al, form):
    assert (form == "mfma") == (K % 128 == 0 and (lay == 1 or al))                 # the entry's own rule, restated
    for cancel in (False, True):
        a, w = _small_rows_data(M, N, K, lay, cancel, 300 + SMALL_ROWS.index((M, N, K, lay, alpha, al, form)))
        want, T = _small_rows_ref(a, w, lay, alpha)
        rc, out = _run_small_rows(a, w, lay, alpha, al, dev)
        assert out.takes == 1 and rc == 0 and out.intact()
        _hold(out.v, want, T, f"small_rows {M}x{N}x{K} {'nn' if lay else 'nt'} {form}", "small_rows, " + form, A_SMALL)
    if form == "mfma" and M > 1:                                                     # non-finite rows stay rows, the last one included
        a, w = a.clone(), w.clone()
        a[M - 1, K - 1], a[0, 1] = NAN, INF
        n3 = N - 1
        if lay:
            w[K // 2, n3] = -INF
        else:
            w[n3, K // 2] = -INF
        want, _ = _small_rows_ref(a, w, lay, alpha)
        rc, out = _run_small_rows(a, w, lay, alpha, al, dev)
        got = out.v.cpu().double()
        assert rc == 0 and out.intact() and torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(got[torch.isinf(want)], want[torch.isinf(want)])
        fa, fw = torch.nan_to_num(a, 0.0, 0.0, 0.0), torch.nan_to_num(w, 0.0, 0.0, 0.0)
        wf, T = _small_rows_ref(fa, fw, lay, alpha)
        ok = torch.isfinite(want)
        assert ((got - wf).abs()[ok] <= A_SMALL * U * T[ok]).all()


def test_small_rows_declines_many_rows_off_the_mfma_form(dev):
    """... and "nn" rows off that form that do not fit its 64 KB of LDS with the partial sums (832 columns of 16 rows do: SMALL_ROWS
    has no such row, so the fit is run here); ops.gemm_own used to send the latter there"""
    for M, N, K, lay, takes in ((64, 16, 100, 0, 0), (16, 8, 833, 1, 0), (16, 8, 1000, 1, 0), (16, 8, 832, 1, 1)):
        a, w = _small_rows_data(M, N, K, lay, False, 1)
        rc, out = _run_small_rows(a, w, lay, 1.0, True, dev)
        assert out.takes == takes and out.intact()
        if takes:
            assert rc == 0
            _hold(out.v, *_small_rows_ref(a, w, lay, 1.0), f"small_rows {M}x{N}x{K} nn lanes", "small_rows, lanes", A_SMALL)
        else:
            assert rc == -2 and torch.isnan(out.v).all()


def _run_outer(a, c, mom, Cm, dev, pair=None):
    """hsp_small_outer_f32, or hsp_small_pair_f32 with pair = (W (Ma, Nn), alpha)"""
    B, Ma = a.shape
    Nb = c.shape[1]
    av, cv = _in_moat(a, Ma + 3, dev), _in_moat(c, Nb + 1, dev)
    out = Out(Ma, Nb, Nb + 1, dev)
    mv = _in_moat(mom, 3 * Cm + 2, dev) if Cm else None
    gs = Out(Cm, 3, 3, dev) if Cm else None
    if pair is None:
        rc = _L().hsp_small_outer_f32(_vp(av), Ma + 3, _vp(cv), Nb + 1, B, Ma, Nb, _vp(out.v), Nb + 1, _vp(mv), 3 * Cm + 2, Cm,
                                      _vp(gs.v if gs else None), _stream())
        onn = None
    else:
        W, alpha = pair
        Nn = W.shape[1]
        wv = _in_moat(W, Nn + 1, dev)
        onn = Out(B, Nn, Nn + 1, dev)
        rc = _L().hsp_small_pair_f32(_vp(av), Ma + 3, B, Ma, _vp(wv), Nn + 1, Nn, alpha, _vp(onn.v), Nn + 1, _vp(cv), Nb + 1, Nb,
                                     _vp(out.v), Nb + 1, _vp(mv), 3 * Cm + 2, Cm, _vp(gs.v if gs else None), _stream())
    torch.cuda.synchronize()
    return rc, out, gs, onn


@pytest.mark.parametrize("B,Ma,Nb,Cm", SMALL_OUTER)
def test_small_outer(dev, B, Ma, Nb, Cm):
    for cancel in (False, True):
        a, c, mom = _outer_data(B, Ma, Nb, Cm, cancel, 400 + SMALL_OUTER.index((B, Ma, Nb, Cm)))
        rc, out, gs, _ = _run_outer(a, c, mom, Cm, dev)
        assert rc == 0 and out.intact() and (gs is None or gs.intact())
        _hold(out.v, a.double().t() @ c.double(), a.double().abs().t() @ c.double().abs(), f"small_outer {B} {Ma}x{Nb}", "small_outer", A_SMALL)
        if Cm:
            _hold(gs.v, *_gste_ref(mom, Cm), f"small_outer {B} gste", "small_outer", A_SMALL)


@pytest.mark.parametrize("B,Ma,Nn,Nb,Cm", SMALL_PAIR)
def test_small_pair(dev, B, Ma, Nn, Nb, Cm):
    for cancel in (False, True):
        a, c, mom = _outer_data(B, Ma, Nb, Cm, cancel, 500 + B)
        g = torch.Generator().manual_seed(600 + B)
        W = _ranged(Ma, Nn, g)
        if cancel:                                                                  # the nn product sums over Ma: cancel along it
            at, wt = a.clone(), W.t().contiguous()
            _cancel_cols(at, wt, g)
            a, W = at, wt.t().contiguous()
        rc, out, gs, onn = _run_outer(a, c, mom, Cm, dev, (W, 0.5))
        assert rc == 0 and out.intact() and onn.intact() and (gs is None or gs.intact())
        _hold(out.v, a.double().t() @ c.double(), a.double().abs().t() @ c.double().abs(), f"small_pair {B} outer", "small_pair", A_SMALL)
        _hold(onn.v, *_small_rows_ref(a, W, 1, 0.5), f"small_pair {B} nn", "small_pair", A_SMALL)
        if Cm:
            _hold(gs.v, *_gste_ref(mom, Cm), f"small_pair {B} gste", "small_pair", A_SMALL)


# ==== the LDS-free wave-level kernel: hsp_gemm_wave_f32 (csrc/gemm_wave.hip) =====================================================
# the contract of hsp_gemm_rows_f32 for K and N multiples of 32 and 16-byte rows; one case per instantiated form, every tile
# configuration of tests/test_gpu_gemm_rows.py; a configuration whose tile does not divide N must be declined

WAVE_CFGS = [0, 0x10042, 0x20041, 0x20021, 0x20011, 0x10020041]
WAVE = [
    R(65, 128, (32, 1), None, "b", 0, 1.0, 16, None),                       # fm: "nn" + bias
    R(33, 128, (64, 1), None, "", 0, 1.0, 16, None),                        # g W: "nn"; two row blocks, one of them a single row
    R(129, 128, (32, 0), None, "", 0, 1.0, 16, None),                      # x W^T
    R(33, 96, (32, 0), None, "", 0, 1.0, 16, None),                        # N = 3 x 32: the wider tiles do not divide it and are declined
    R(63, 128, (96, 0), None, "b", 0, 1.0, 16, None),                      # x W^T + b
    R(129, 128, (32, 0), (64, 0), "rc", 100, 1.0, 16, None),                # out: two sources, residual + cloud bias, a short last cloud
    R(65, 128, (32, 0), None, "rcx", 64, 1.0, 16, None),                    # out0: + the xyz3 rider; the last cloud is one row
    R(64, 128, (32, 1), (96, 0), "", 0, 1.0, 16, None),                     # gX: "nn" + "nt"
]


def _run_wave(c, d, cfg, dev):
    L = _L()
    ops_ = []
    for a, b, lay, K in d.src:
        av, bv = _in_moat(a, K + 4, dev), _in_moat(b, b.shape[1] + 4, dev)
        ops_.append((av, av.stride(0), bv, bv.stride(0), lay, K))
    if len(ops_) == 1:
        ops_.append((None, 0, None, 0, 0, 0))
    out = Out(c.M, c.N, c.N + 4, dev)
    resid = _in_moat(d.resid, c.N + 4, dev) if d.resid is not None else None
    bias = _in_moat(d.bias[None], c.N, dev) if d.bias is not None else None
    cb = _in_moat(d.cb, c.N, dev) if d.cb is not None else None
    xyz = _in_moat(d.xyz, 3, dev) if d.xyz is not None else None
    w3 = _in_moat(d.w3, 3, dev) if d.w3 is not None else None
    (a1, la1, b1, lb1, l1, K1), (a2, la2, b2, lb2, l2, K2) = ops_
    out.takes = _takes(gc.WAVE, c.M, c.N, [(a1, b1, l1, K1)] + ([(a2, b2, l2, K2)] if a2 is not None else []), out.v, resid, bias, cb, xyz,
                       c.alpha, c.rpc)
    rc = L.hsp_gemm_wave_f32(_vp(a1), la1, _vp(b1), lb1, l1, K1, _vp(a2), la2, _vp(b2), lb2, l2, K2, c.M, c.N, _vp(bias), _vp(resid),
                             c.N + 4, _vp(cb), c.rpc, c.alpha, _vp(xyz), _vp(w3), _vp(out.v), c.N + 4, cfg, _stream())
    torch.cuda.synchronize()
    return rc, out


def test_fp32_composition_sets_A_wave():
    """the same rule for the wave kernel's cases.  (Needs no GPU.)"""
    worst = 0.0
    for c in WAVE:
        for cancel in (False, True):
            d, want, T = _rows_case(c, cancel)
            worst = max(worst, _ratio("composition wave", (_rows_ref(c, d, torch.float32)[0].double() - want).abs(), T))
    print(f"  composition ratio, wave: {worst:.3f}")
    rule = 2.0 ** np.ceil(np.log2(4 * worst))
    assert rule <= A_WAVE <= 2 * rule, f"the composition's worst ratio {worst:.3f} asks for A = {rule}"


@pytest.mark.parametrize("cfg", WAVE_CFGS, ids=hex)
@pytest.mark.parametrize("c", WAVE, ids=_rid)
def test_gemm_wave_f32(dev, c, cfg):
    L = _L()
    K1, K2 = c.s1[0], c.s2[0] if c.s2 else 0
    info = (ctypes.c_int * 10)()
    ok = L.hsp_gemm_wave_plan_info(c.M, c.N, K1, K2, cfg, info)
    assert bool(ok) == bool(L.hsp_gemm_wave_supported(c.M, c.N, K1, K2, cfg))
    if ok:
        RB, NCB, wps, TM, TN = info[0], info[1], info[2], info[3], info[4]
        if cfg:
            assert (RB, NCB, wps) == (cfg & 15, (cfg >> 4) & 15, (cfg >> 16) & 15), "the plan is not the configuration asked for"
        assert TM == -(-c.M // (32 * RB)) and TN * 32 * NCB == c.N
    else:
        assert cfg and c.N % (32 * ((cfg >> 4) & 15)), "declined although the tile divides N"
    for cancel in (False, True):
        d, want, T = _rows_case(c, cancel)
        rc, out = _run_wave(c, d, cfg, dev)
        what = f"wave {_rid(c)} cfg {cfg:#x} {'cancel' if cancel else 'range'}"
        if not ok:
            assert rc == -2 and out.intact() and torch.isnan(out.v).all(), f"{what}: not declined cleanly"
            continue
        assert rc == 0 and out.intact(), f"{what}: rc {rc}, or a write outside the output"
        assert cfg or out.takes == 1, f"{what}: hsp_gemm_takes declines what the entry point ran"      # (the query knows no forced tile)
        _hold(out.v, want, T, what, "gemm_wave", A_WAVE)


# calls gw_plan cuts that the kernel has no form for, or whose clouds are shorter than a tile: a residual alone, bias + the out
# product's riders, "nt" + "nn", clouds of 31 rows
WAVE_REFUSED = [R(129, 128, (32, 0), None, "r", 0, 1.0, 16, None), R(129, 128, (32, 0), (64, 0), "brc", 100, 1.0, 16, None),
                R(64, 128, (32, 0), (96, 1), "", 0, 1.0, 16, None), R(129, 128, (32, 0), (64, 0), "rc", 31, 1.0, 16, None)]


@pytest.mark.parametrize("c", WAVE_REFUSED, ids=_rid)
def test_gemm_wave_declines_what_its_query_declines(dev, c):
    assert _L().hsp_gemm_wave_supported(c.M, c.N, c.s1[0], c.s2[0] if c.s2 else 0, 0) == 1
    rc, out = _run_wave(c, _rows_data(c, 1, False, torch.float32), 0, dev)
    assert out.takes == 0 and rc == -2 and out.intact() and torch.isnan(out.v).all()


@pytest.mark.parametrize("edge", [False, True], ids=["inside", "last-rows"])
def test_gemm_wave_nonfinite_is_confined(dev, edge):
    c = WAVE[5]
    d0, _, _ = _rows_case(c, False)
    d = SimpleNamespace(**vars(d0))
    d.src = [(a.clone(), b.clone(), lay, K) for a, b, lay, K in d0.src]
    M, N, K1, Kl = c.M, c.N, d.src[0][3], d.src[-1][3]
    (r1, k1), (r2, k2), (n3, k3) = ((M - 1, K1 - 1), (M - 2, 0), (N - 1, Kl - 1)) if edge else ((M // 3, K1 // 2), (M // 2, 1), (N // 2, Kl // 3))
    d.src[0][0][r1, k1], d.src[0][0][r2, k2], d.src[-1][1][n3, k3] = NAN, INF, -INF
    want, _ = _rows_ref(c, d)
    bad = ~torch.isfinite(want)
    assert int(bad.sum()) == 2 * N + M - 2
    fin = SimpleNamespace(**vars(d))
    fin.src = [(torch.nan_to_num(a, 0.0, 0.0, 0.0), torch.nan_to_num(b, 0.0, 0.0, 0.0), lay, K) for a, b, lay, K in d.src]
    wfin, T = _rows_ref(c, fin)
    rc, out = _run_wave(c, d, 0, dev)
    got = out.v.cpu().double()
    assert rc == 0 and out.intact() and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got[torch.isinf(want)], want[torch.isinf(want)])
    assert ((got - wfin).abs()[~bad] <= A_WAVE * U * T[~bad]).all()


def test_zz_measured_ratios():
    print("\n  measured err / (2^-24 T), worst over this run:")
    for k in sorted(RATIOS):
        print(f"  {k:44s} {RATIOS[k]:.3f}")
