"""numpy RESTATEMENT of hsp_sample_ids, written from the text of include/hsp.h (section "the rows each instance keeps, drawn
on the device"), not from the kernel: uint32 arithmetic that wraps, the same constants, key schedule and order of operations.
What the kernel is held to bit for bit (tests/test_gpu_sample_ids.py) and what the distribution checks run on
(tests/test_sample_ids_host.py)."""
import numpy as np

_U32 = np.uint32


def fmix32(h):
    h = np.array(h, dtype=_U32, ndmin=1)
    h ^= h >> _U32(16)
    h *= _U32(0x85ebca6b)
    h ^= h >> _U32(13)
    h *= _U32(0xc2b2ae35)
    h ^= h >> _U32(16)
    return h


def absorb(h, w):
    return fmix32((np.array(h, dtype=_U32, ndmin=1) ^ np.array(w, dtype=_U32, ndmin=1)) + _U32(0x9e3779b9))


def instance_key(seed, call, j):
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    k = absorb(0, seed & 0xffffffff)
    k = absorb(k, seed >> 32)
    k = absorb(k, call & 0xffffffff)
    k = absorb(k, call >> 32)
    return absorb(k, j)


def half_bits(c):
    bits = 0 if c <= 1 else int(c - 1).bit_length()
    return max(1, (bits + 1) // 2)


def one_pass(x, half, k):
    mask, hs = _U32((1 << half) - 1), _U32(half)
    L, R = x >> hs, x & mask
    for r in range(4):
        L, R = R, L ^ (fmix32(R ^ k[r]) & mask)
    return (L << hs) | R


def permute(xs, c, kj):
    """P(x) for every x of xs (values below c)"""
    half = half_bits(c)
    k = [absorb(kj, r) for r in range(4)]
    x = one_pass(np.array(xs, dtype=_U32, ndmin=1), half, k)
    while True:
        walk = x >= _U32(c)
        if not walk.any():
            return x.astype(np.int64)
        x[walk] = one_pass(x[walk], half, k)


def sample_ids(counts, S, seed, call, min_pts, min_depth_pts=0, short_mode=0):
    """counts (n,) or (n,2) -> (choose (n,S) int32, status (n,) int32)"""
    counts = np.asarray(counts)
    n = counts.shape[0]
    choose = np.full((n, S), -1, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    s = np.arange(S)
    for j in range(n):
        c = int(counts[j, 0] if counts.ndim == 2 else counts[j])
        status[j] = (1 if c < min_pts else 0) | (2 if counts.ndim == 2 and int(counts[j, 1]) < min_depth_pts else 0)
        if status[j] != 0 or c <= 0:
            continue
        if short_mode == 0 and c <= S:
            choose[j] = s % c
        elif short_mode == 1 and c < S:
            h = absorb(absorb(instance_key(seed, call, j), 0xffffffff), s)
            choose[j] = ((h.astype(np.uint64) * np.uint64(c)) >> np.uint64(32)).astype(np.int32)
        else:
            choose[j] = permute(s, c, instance_key(seed, call, j))
    return choose, status
