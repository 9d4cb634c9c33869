"""Host-side checks of the two restatements the reproducible step is held to (tests/_dropout_ref.py, tests/_pool_bwd_ref.py): the
keyed Dropout keeps at the rate it should and its streams are apart, and the pooling restatement's inputs are ones on which
another summation order changes bits -- so the GPU test's bit-equality (tests/test_gpu_pool_bwd_ordered.py) can tell one order
from another.  Plus what needs no GPU of the new entry points: their bad-argument codes (nothing is launched)."""
import ctypes
import math

import numpy as np
import pytest

import _dropout_ref as dref
import _pool_bwd_ref as pref

SEED = 0x9e3779b97f4a7c15


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_keep_rate(p):
    n = 2 ** 16
    keep = dref.keep_mask(SEED, 3, 0, p, 256, 256)
    rate, se = keep.mean(), math.sqrt(p * (1 - p) / n)
    assert abs(rate - (1 - p)) <= 5 * se, (rate, se)


def test_sites_and_calls_differ():
    a = dref.keep_mask(SEED, 3, 0, 0.5, 16, 256)
    assert not np.array_equal(a, dref.keep_mask(SEED, 3, 1, 0.5, 16, 256))
    assert not np.array_equal(a, dref.keep_mask(SEED, 4, 0, 0.5, 16, 256))
    assert np.array_equal(a, dref.keep_mask(SEED, 3, 0, 0.5, 16, 256))
    # a prefix property of the word stream: element i does not depend on the shape it is cut into
    assert np.array_equal(a.reshape(-1)[:1024], dref.keep_mask(SEED, 3, 0, 0.5, 4, 256).reshape(-1))


def test_dropout_values():
    x = np.linspace(-2, 2, 3 * 256, dtype=np.float32).reshape(3, 256)
    out, keep = dref.dropout(x, SEED, 2 ** 32 + 1, 2, 0.2)
    assert out.dtype == np.float32 and keep.dtype == np.uint8 and set(np.unique(keep)) == {0, 1}
    assert np.array_equal(out[keep == 0], np.zeros((keep == 0).sum(), np.float32))
    assert np.array_equal(out[keep == 1], (x * dref.scale_of(0.2))[keep == 1])
    out0, keep0 = dref.dropout(x, SEED, 0, 0, 0.0)
    assert keep0.all() and np.array_equal(out0, x)


def test_bf16_rounding_helper():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0, 3.0e38], np.float32)
    got = pref.bf16_value(pref.bf16_bits(x))
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -0.0, 3.0e38], np.float32)      # ties to even, then above a tie
    assert np.array_equal(got[:5].view(np.uint32), want[:5].view(np.uint32))
    assert abs(float(got[5]) - 3.0e38) <= 3.0e38 * 2.0 ** -8


@pytest.mark.parametrize("indeg,least", [(4, 0.2), (64, 0.6)])
def test_order_changes_bits(indeg, least):
    """in-degree Nq k / (k Nsrc) per (row, column) cell: Nq queries, each column of a query lands on one of Nsrc rows"""
    Nsrc, k, C = 8, 4, 32
    g, idx, argmax = pref.order_case(2, Nsrc, indeg * Nsrc, k, C, 11 + indeg)
    up = pref.pool_bwd(g, idx, argmax, None, Nsrc)
    down = pref.pool_bwd(g, idx, argmax, None, Nsrc, descending=True)
    differ = (up.view(np.uint32) != down.view(np.uint32)).mean()
    print(f"in-degree {indeg}: {100 * differ:.0f} % of the cells differ between ascending and descending order")
    assert differ >= least, differ
    assert np.allclose(up, down, rtol=1e-4, atol=1e-4 * np.abs(g).max())             # the same sum, another rounding
    # (after a bf16 store the two orders agree almost everywhere: the store hides the last fp32 bits unless the sum sits at a
    # rounding tie, so the bf16 GPU cases check the routing, the fp32 accumulation and the single rounding, the fp32 cases the order)


def test_rev_index_restatement():
    rng = np.random.RandomState(5)
    idx = rng.randint(0, 19, size=(2, 12, 5)).astype(np.int32)
    qsel = np.array([[3, 3, 0, 11], [7, 1, 1, 2]], np.int32)
    off, edge = pref.rev_index(idx, qsel, 19, 4)
    for b in range(2):
        assert off[b, 0] == 0 and off[b, -1] == 16
        for m in range(19):
            lst = edge[b, off[b, m]:off[b, m + 1]]
            assert list(lst) == sorted(lst)
            assert list(lst) == [q * 4 + n for q in range(4) for n in range(4) if idx[b, qsel[b, q], n] == m]


def _lib():
    from hs_pose_amd import _lib
    return _lib.lib(), _lib.CONSTANTS                   # (a missing library is a hard error, not a skip)


def test_bad_arguments_launch_nothing():
    """every refusal below returns before anything touches the device: the pointers are never read"""
    L, K = _lib()
    bad, uns = K["ERR_BAD_ARG"], K["ERR_UNSUPPORTED"]
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    # hsp_rev_build_sel(idx, qsel, qsel_stride, B, Nidx, Nq, Nsrc, k, kstride, rev_off, rev_edge, stream)
    assert L.hsp_rev_build_sel(null, one, 0, 1, 8, 4, 8, 4, 4, one, one, null) == bad
    assert L.hsp_rev_build_sel(one, one, 0, 1, 8, 4, 8, 4, 4, null, one, null) == bad
    assert L.hsp_rev_build_sel(one, one, 0, 0, 8, 4, 8, 4, 4, one, one, null) == bad          # B
    assert L.hsp_rev_build_sel(one, one, 0, 1, 8, 0, 8, 4, 4, one, one, null) == bad          # Nq
    assert L.hsp_rev_build_sel(one, one, 0, 1, 8, 4, 8, 4, 3, one, one, null) == bad          # kstride < k
    assert L.hsp_rev_build_sel(one, one, 3, 1, 8, 4, 8, 4, 4, one, one, null) == bad          # 0 < stride < Nq
    assert L.hsp_rev_build_sel(one, null, 4, 1, 8, 8, 8, 4, 4, one, one, null) == bad         # a stride without a list
    assert L.hsp_rev_build_sel(one, null, 0, 1, 8, 4, 8, 4, 4, one, one, null) == bad         # no list: Nq must be Nidx
    assert L.hsp_rev_build_sel(one, one, 0, 1, 8, 4, 40000, 4, 4, one, one, null) == uns      # the histogram's LDS
    # hsp_gather_max_bwd_csr_bf16(grad_out, grad_bcast, argmax, rev_off, rev_edge, B, Nsrc, Nq, k, C, grad_feat, stream)
    for fn in (L.hsp_gather_max_bwd_csr, L.hsp_gather_max_bwd_csr_bf16):
        assert fn(one, 0, one, one, one, 1, 8, 8, 4, 126, one, null) == uns                   # C % 4
        assert fn(null, 0, one, one, one, 1, 8, 8, 4, 128, one, null) == bad
        assert fn(one, 0, one, one, one, 1, 8, 8, 4, 128, null, null) == bad
        assert fn(one, 0, one, one, one, 1, 0, 8, 4, 128, one, null) == bad
        assert fn(one, 0, one, one, one, 1, 8, 8, 0, 128, one, null) == bad
    # hsp_dropout_keyed_fwd(x, key, site, p, R, C, out, keep, stream)
    assert L.hsp_dropout_keyed_fwd(null, one, 0, 0.2, 1, 4, one, one, null) == bad
    assert L.hsp_dropout_keyed_fwd(one, null, 0, 0.2, 1, 4, one, one, null) == bad
    assert L.hsp_dropout_keyed_fwd(one, one, 0, 1.0, 1, 4, one, one, null) == bad             # p = 1
    assert L.hsp_dropout_keyed_fwd(one, one, 0, -0.1, 1, 4, one, one, null) == bad
    assert L.hsp_dropout_keyed_fwd(one, one, 0, float("nan"), 1, 4, one, one, null) == bad
    assert L.hsp_dropout_keyed_fwd(one, one, 1 << 24, 0.2, 1, 4, one, one, null) == bad       # site
    assert L.hsp_dropout_keyed_fwd(one, one, -1, 0.2, 1, 4, one, one, null) == bad
    assert L.hsp_dropout_keyed_fwd(one, one, 0, 0.2, 0, 4, one, one, null) == bad
    assert L.hsp_dropout_keyed_fwd(one, one, 0, 0.2, 65536, 65536, one, one, null) == bad     # R C = 2^32
    assert L.hsp_dropout_bwd(one, null, 0.2, 1, 4, one, null) == bad
    assert L.hsp_dropout_bwd(one, one, 1.0, 1, 4, one, null) == bad


def test_flag_default_and_reset():
    from hs_pose_amd.config import FLAGS
    FLAGS.reset()
    assert FLAGS.reproducible is False
    FLAGS.reproducible = True
    FLAGS.reset()
    assert FLAGS.reproducible is False
