"""numpy RESTATEMENT of the ordered pooling backward, written from the contract in include/hsp.h (hsp_gather_max_bwd_csr /
hsp_gather_max_bwd_csr_bf16 over hsp_rev_build_sel), not from the kernels: for every cloud, source row and column one fp32 sum
from +0 over the queries in ascending order, each add rounded to fp32, stored as is (fp32) or rounded once to nearest even
(bf16).  ``rev_index`` is the numpy inversion hsp_rev_build_sel is held to.  What tests/test_gpu_pool_bwd_ordered.py compares the
kernels with bit for bit, and what tests/test_reproducible_host.py shows to be sensitive to the order."""
import numpy as np


def bf16_bits(x):
    """fp32 array -> the bf16 bits (uint16) of each value, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    """bf16 bits (uint16) -> the fp32 values they stand for"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def kept_rows(qsel, B, Nidx):
    """the (B,Nq) idx row every query reads: qsel None (identity), (Nq,) shared by the batch, or (B,Nq) per cloud"""
    if qsel is None:
        return np.broadcast_to(np.arange(Nidx), (B, Nidx))
    qsel = np.asarray(qsel)
    return np.broadcast_to(qsel, (B, qsel.shape[-1])) if qsel.ndim == 1 else qsel


def pool_bwd(grad_out, idx, argmax, qsel, Nsrc, descending=False):
    """grad_out (B,Nq,C) fp32 VALUES (a bf16 gradient: its values), idx (B,Nidx,kstride) ints, argmax (B,Nq,C) uint8 ->
    grad_feat (B,Nsrc,C) fp32 before the store.  ``descending``: the same sum taken from the last query to the first (the host
    test's other order)."""
    g = np.asarray(grad_out, dtype=np.float32)
    B, Nq, C = g.shape
    rows = kept_rows(qsel, B, idx.shape[1])
    out = np.zeros((B, Nsrc, C), np.float32)                       # s = +0
    cols = np.arange(C)
    for b in range(B):
        for q in (range(Nq - 1, -1, -1) if descending else range(Nq)):
            m = idx[b, rows[b, q], argmax[b, q]]                   # (C,): the winning source row of every column
            out[b, m, cols] = (out[b, m, cols] + g[b, q]).astype(np.float32)      # distinct cells: one fp32 add each
    return out


def rev_index(idx, qsel, Nsrc, k):
    """(rev_off (B,Nsrc+1), rev_edge (B,Nq*k)) int32: for source row m the ascending edge ids e = q*k + n with
    idx[b, r_q, n] == m"""
    B = idx.shape[0]
    rows = kept_rows(qsel, B, idx.shape[1])
    Nq = rows.shape[1]
    off = np.zeros((B, Nsrc + 1), np.int32)
    edge = np.empty((B, Nq * k), np.int32)
    for b in range(B):
        src = idx[b, rows[b], :k].reshape(-1)                      # source row of edge e = q*k + n
        order = np.argsort(src, kind="stable")                     # by source row, ascending edge id within a row
        edge[b] = order
        off[b, 1:] = np.cumsum(np.bincount(src, minlength=Nsrc))
    return off, edge


def order_case(B, Nsrc, Nq, k, C, seed):
    """inputs on which the order of the sum matters: arg-max bytes uniform in [0, k), lists uniform over the source rows,
    gradients randn * 2^U{-8..8}"""
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, Nsrc, size=(B, Nq, k)).astype(np.int32)
    argmax = rng.randint(0, k, size=(B, Nq, C)).astype(np.uint8)
    g = (rng.randn(B, Nq, C) * 2.0 ** rng.randint(-8, 9, size=(B, Nq, C))).astype(np.float32)
    return g, idx, argmax
