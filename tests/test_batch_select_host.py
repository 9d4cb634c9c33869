"""hsp_batch_select without a GPU: the properties of the rule on its numpy restatement (tests/_batch_select_ref.py, written
from include/hsp.h) and the entry point's argument checks through libhsp.so, each HSP_ERR_BAD_ARG before any launch."""
import ctypes

import numpy as np
import pytest

import _batch_select_ref as br


def _cases():
    rng = np.random.RandomState(5)
    out = [([0], 1), ([0, 0, 0, 0], 4), ([0, 1, 0, 4, 0, 0], 4), ([2, 0, 1, 4, 0, 3], 4), ([0, 0, 0, 0, 7, -1], 4),
           ([1, 2, 4, 7, -1], 4), ([0, 3, 0, 0, 5], 4), ([0, 3, 0, 0, 0], 4)]
    for M in (63, 64, 65, 129, 1024):
        st = br.random_status(rng, M)
        out += [(st.tolist(), keep) for keep in (1, M // 2, M)]
    return out


@pytest.mark.parametrize("status,keep", _cases())
def test_rule_properties(status, keep):
    sel, info = br.select(status, keep)
    st = np.asarray(status)
    V = int((st == 0).sum())
    assert sel.shape == (keep,) and sel.dtype == np.int32 and info.tolist() == [V, min(V, keep)]
    assert ((sel >= 0) & (sel < len(st))).all()
    if V == 0:
        assert sel.tolist() == list(range(keep))                      # the identity
        return
    assert (st[sel] == 0).all()                                       # never a rejected item
    if V >= keep:
        assert (np.diff(sel) > 0).all()                               # ascending, hence duplicate-free
        assert sel.tolist() == np.flatnonzero(st == 0)[:keep].tolist()   # the FIRST keep good items: later spares untouched
    else:
        assert np.array_equal(sel[V:], sel[:keep - V])                # period V
        assert sel[:V].tolist() == np.flatnonzero(st == 0).tolist()


def test_gather_moves_bytes():
    rng = np.random.RandomState(1)
    src = rng.randn(6, 5, 3).astype(np.float32)
    src[1] = np.nan
    src.view(np.uint32)[3, 0, 0] = 0x7fc12345                          # a NaN payload passes unchanged
    sel, info = br.select([0, 1, 0, 0, 0, 0], 4)
    got = br.gather(src, sel, info[0])
    assert np.array_equal(got.view(np.uint32), src[[0, 2, 3, 4]].view(np.uint32))
    fill = np.full((5, 3), 2.5, np.float32)
    sel, info = br.select([1] * 6, 4)
    assert np.array_equal(br.gather(src, sel, info[0], fill), np.stack([fill] * 4))
    assert np.array_equal(br.gather(src, sel, info[0]).view(np.uint32), src[:4].view(np.uint32))


def test_argument_validation_without_gpu():
    from hs_pose_amd._lib import BATCH_SELECT_MAX_ITEMS, BATCH_SELECT_MAX_SEGS, HspSelectSeg, lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    assert (BATCH_SELECT_MAX_SEGS, BATCH_SELECT_MAX_ITEMS) == (16, 1024)
    segs = (HspSelectSeg * 17)()
    for s in range(17):
        segs[s] = HspSelectSeg(1 << 20, 2 << 20, None, 16)

    def call(status=one, M=8, keep=4, segs=segs, nseg=2, sel=one, info=one):
        return L.hsp_batch_select(status, M, keep, segs, nseg, sel, info, null)

    assert call(keep=0) == -1
    assert call(keep=9) == -1                                         # keep > M
    assert call(M=1025, keep=4) == -1 and call(M=1025, keep=1025) == -1
    assert call(nseg=17) == -1 and call(nseg=-1) == -1
    assert call(status=null) == -1 and call(sel=null) == -1 and call(info=null) == -1
    assert call(segs=None, nseg=1) == -1
    for bad in (HspSelectSeg(1 << 20, 2 << 20, None, 6), HspSelectSeg(1 << 20, 2 << 20, None, 0),
                HspSelectSeg(1 << 20, 2 << 20, None, -4), HspSelectSeg(None, 2 << 20, None, 16),
                HspSelectSeg(1 << 20, None, None, 16), HspSelectSeg((1 << 20) + 2, 2 << 20, None, 16),
                HspSelectSeg(1 << 20, 2 << 20, (3 << 20) + 1, 16),
                HspSelectSeg(1 << 20, (1 << 20) + 64, None, 16)):          # dst inside src
        two = (HspSelectSeg * 2)(segs[0], bad)
        assert call(segs=two) == -1, (bad.src, bad.dst, bad.fill, bad.row_bytes)


def test_header_states_the_rule_and_table_lists_the_entry():
    import os
    from hs_pose_amd import _lib
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hsp.h")).read()
    assert "hsp_batch_select" in _lib.SIGNATURES and "int hsp_batch_select(" in txt
    assert "sel[j] = v_{j mod V}" in txt and "#define HSP_BATCH_SELECT_MAX_SEGS 16" in txt
    assert "#define HSP_BATCH_SELECT_MAX_ITEMS 1024" in txt
