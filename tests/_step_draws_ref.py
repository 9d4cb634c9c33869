"""numpy RESTATEMENT of the keyed draws of a step, written from the text of include/hsp.h (section "keyed draws of a step"),
not from the kernels: the streams' instance indices and tags, the two word-to-uniform conversions, and the float64 arithmetic of
the DZI windows step by step.  fmix32 / absorb / the instance key / the permutation P are hsp_sample_ids's
(tests/_sample_ids_ref.py).  What the kernels are held to bit for bit (tests/test_gpu_step_draws.py) and what the distribution
checks run on (tests/test_step_draws_host.py)."""
import numpy as np

from _sample_ids_ref import absorb, instance_key, permute

POOL_J, AUG_J, DZI_J = 0x80000000, 0x81000000, 0x82000000
AUG_TAG, DZI_TAG = 0xfffffffc, 0xfffffffb


def words(kj, tag, idx):
    """word(i) = absorb(absorb(kj, tag), i) for every i of idx -> uint32"""
    return absorb(absorb(kj, tag), np.asarray(idx, dtype=np.uint32))


def uniform_f32(w):
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def uniform_f64(w):
    return np.asarray(w, dtype=np.uint32).astype(np.float64) * 2.0 ** -32


def pool_rows(seed, call, n0, rate=4, levels=2):
    """-> [rows of level 0, (rows of level 1)], int32: level l keeps the first n_l // rate values of P over [0, n_l)"""
    out, n = [], int(n0)
    for level in range(levels):
        m = n // rate
        out.append(permute(np.arange(m), n, instance_key(seed, call, POOL_J | level)).astype(np.int32))
        n = m
    return out


def augment_draws(seed, call, B, N, aug_pc_r):
    """-> (draws (6,B) float32, noise (B,N,3) float32): what hsp_pose_augment_keyed draws, in hsp_pose_augment's layout"""
    draws = np.empty((6, B), np.float32)
    noise = np.empty((B, N * 3), np.float32)
    for b in range(B):
        kb = instance_key(seed, call, AUG_J | b)
        draws[:, b] = uniform_f32(words(kb, AUG_TAG, np.arange(6)))
        noise[b] = uniform_f32(words(kb, AUG_TAG, 6 + np.arange(3 * N))) * np.float32(aug_pc_r)
    return draws, noise.reshape(B, N, 3)


def dzi_uniforms(seed, call, M):
    """-> (M,3) float64: u0, u1, u2 of every item"""
    return np.stack([uniform_f64(words(instance_key(seed, call, DZI_J | i), DZI_TAG, np.arange(3))) for i in range(M)])


def dzi_xf(bboxes, seed, call, H, W, out_size, pad_scale, scale_ratio, shift_ratio):
    """bboxes (M,4) integers (x1, y1, x2, y2) -> xf (M,3) float64, every operation of the header's list in its order"""
    boxes = np.asarray(bboxes, dtype=np.int64)
    u = dzi_uniforms(seed, call, len(boxes))
    f = np.float64
    xf = np.empty((len(boxes), 3), np.float64)
    for i, (x1, y1, x2, y2) in enumerate(boxes):
        cx, cy = f(0.5) * f(x1 + x2), f(0.5) * f(y1 + y2)
        bw, bh = f(x2 - x1), f(y2 - y1)
        sr = f(1) + f(scale_ratio) * (f(2) * u[i, 0] - f(1))
        sx = f(shift_ratio) * (f(2) * u[i, 1] - f(1))
        sy = f(shift_ratio) * (f(2) * u[i, 2] - f(1))
        cx2, cy2 = cx + bw * sx, cy + bh * sy
        scale = min((max(bh, bw) * sr) * f(pad_scale), f(max(H, W)))
        O = f(out_size)
        a = O / scale
        tx, ty = O / f(2) - a * cx2, O / f(2) - a * cy2
        D = f(1) / (a * a)
        m0 = a * D
        xf[i] = m0, (-m0) * tx, (-m0) * ty
    return xf
