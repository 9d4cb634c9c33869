"""numpy restatement of hsp_batch_select's rule, written from the text in include/hsp.h and independent of the kernel:

  V = the number of items with status 0, v_0 < ... < v_{V-1} those items in ascending order; info = {V, min(V, keep)}
  V >= 1: sel[j] = v_{j mod V};  V == 0: sel[j] = j, and a segment with a fill row gets that row in every dst row
  dst[j] = src[sel[j]] byte for byte
"""
import numpy as np


def select(status, keep):
    """-> (sel (keep,) int32, info (2,) int32)"""
    status = np.asarray(status)
    M = len(status)
    assert 1 <= keep <= M
    good = [i for i in range(M) if int(status[i]) == 0]
    V = len(good)
    sel = [good[j % V] if V else j for j in range(keep)]
    return np.array(sel, dtype=np.int32), np.array([V, min(V, keep)], dtype=np.int32)


def gather(src, sel, V, fill=None):
    """src (M, ...) -> dst (keep, ...), as bytes: nothing is computed on the rows"""
    src = np.ascontiguousarray(src)
    M = src.shape[0]
    rows = src.view(np.uint8).reshape(M, -1)
    if V == 0 and fill is not None:
        one = np.ascontiguousarray(fill).view(np.uint8).reshape(-1)
        assert one.size == rows.shape[1]
        out = np.stack([one] * len(sel))
    else:
        out = np.stack([rows[int(i)] for i in sel])
    return out.view(src.dtype).reshape((len(sel),) + src.shape[1:])


def random_status(rng, M, rate=0.3):
    """seeded status with the given rejection rate: the non-zero values take every form (bits 1, 2, 4, sums, negative)"""
    bad = np.array([1, 2, 4, 7, 3, -1, -2 ** 31, 2 ** 30], dtype=np.int64)
    st = np.where(rng.rand(M) < rate, bad[rng.randint(0, len(bad), size=M)], 0)
    return st.astype(np.int32)
