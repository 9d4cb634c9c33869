"""CPU: the keyed draws of a step (include/hsp.h: "keyed draws of a step") through their numpy restatement
(tests/_step_draws_ref.py) -- the Pool rows are a uniformly drawn ordered subset, the uniforms are uniform, the streams of the
purposes are apart, the DZI arithmetic is the host's -- and the host half of the surface: config.FLAGS.step_draws,
pc_sample.resolve_draws, argument checks that launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

import _sample_ids_ref as sr
import _step_draws_ref as dr

SEED = 0x9e3779b97f4a7c15                                                        # (high bits set)


@pytest.mark.parametrize("n0", [16, 19, 64, 257, 1028])
def test_pool_rows_are_distinct_and_in_range(n0):
    for call in (0, 5, 2 ** 32 + 3):
        rows = dr.pool_rows(SEED, call, n0)
        n = n0
        for r in rows:
            assert r.dtype == np.int32 and len(r) == n // 4
            assert r.min() >= 0 and r.max() < n and len(set(r.tolist())) == len(r)
            n //= 4
    assert [len(r) for r in dr.pool_rows(1, 0, 16)] == [4, 1]
    assert len(dr.pool_rows(1, 0, 1028, levels=1)) == 1


@pytest.mark.parametrize("n,m", [(1028, 257), (257, 64), (64, 16)])
def test_pool_rows_are_a_uniform_ordered_subset(n, m):
    """over calls 0 .. 4095 of one seed: every row is kept equally often, and every row comes first equally often -- the
    chi-square statistic per degree of freedom of either count lies within 5 standard deviations (sqrt(2 / n)) of 1"""
    T = 4096
    kept, first = np.zeros(n), np.zeros(n)
    for call in range(T):
        rows = sr.permute(np.arange(m), n, sr.instance_key(7, call, dr.POOL_J))
        kept[rows] += 1
        first[rows[0]] += 1
    band = 5 * np.sqrt(2.0 / n)
    for obs, p in ((kept, m / n), (first, 1.0 / n)):
        stat = ((obs - T * p) ** 2 / (T * p * (1 - p))).sum() / n
        assert abs(stat - 1) <= band, (n, m, p, stat, band)


def _moments_ok(u):
    n = u.size
    assert u.min() >= 0 and u.max() < 1
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / n), u.mean()
    assert abs(((u - 0.5) ** 2).mean() - 1 / 12) <= 5 * np.sqrt(1 / 180 / n)     # Var((U - 1/2)^2) = 1/80 - 1/144 = 1/180


def test_uniforms():
    draws, noise = dr.augment_draws(SEED, 3, 64, 1028, 1.0)
    assert draws.dtype == noise.dtype == np.float32
    _moments_ok(draws.astype(np.float64))
    _moments_ok(noise.astype(np.float64))
    for q in range(6):                                                           # each of the six per-item uniforms on its own
        _moments_ok(np.concatenate([dr.augment_draws(SEED, c, 64, 1, 1.0)[0][q] for c in range(32)]).astype(np.float64))
    _moments_ok(np.concatenate([dr.dzi_uniforms(SEED, c, 64) for c in range(64)]))
    # the conversions are exact: the fp32 uniform is a multiple of 2^-24 below 1, the float64 one of 2^-32
    w = np.array([0, 1, 255, 256, 0xffffffff, 0xffffff00, 0x80000000], dtype=np.uint32)
    assert dr.uniform_f32(w).tolist() == [0, 0, 0, 2.0 ** -24, 1 - 2.0 ** -24, 1 - 2.0 ** -24, 0.5]
    assert dr.uniform_f64(w).tolist() == [int(x) / 2.0 ** 32 for x in w]
    # the jitter factor is the uniform times r in fp32, one rounding
    _, n2 = dr.augment_draws(SEED, 3, 2, 8, 0.2)
    assert np.array_equal(n2, dr.augment_draws(SEED, 3, 2, 8, 1.0)[1] * np.float32(0.2))


def test_streams_of_different_purposes_differ():
    key = (SEED, 11)
    ks = [int(sr.instance_key(*key, j)[0]) for j in (0, 1, dr.POOL_J, dr.POOL_J | 1, dr.AUG_J, dr.AUG_J | 1, dr.DZI_J, dr.DZI_J | 1)]
    assert len(set(ks)) == len(ks)
    idx = np.arange(64)
    streams = [
        sr.absorb(sr.absorb(sr.instance_key(*key, 0), 0xffffffff), idx),         # a row draw with replacement of instance 0
        dr.words(sr.instance_key(*key, dr.AUG_J), dr.AUG_TAG, idx),
        dr.words(sr.instance_key(*key, dr.AUG_J | 1), dr.AUG_TAG, idx),
        dr.words(sr.instance_key(*key, dr.DZI_J), dr.DZI_TAG, idx),
        dr.words(sr.instance_key(*key, dr.DZI_J | 1), dr.DZI_TAG, idx),
    ]
    for a in range(len(streams)):
        for b in range(a + 1, len(streams)):
            assert (streams[a] == streams[b]).sum() <= 1, (a, b)
    # the two Pool levels and the row draw of instance 0 permute the same domain differently; calls and seeds separate as well
    perms = [sr.permute(idx, 64, sr.instance_key(*key, j)) for j in (0, dr.POOL_J, dr.POOL_J | 1)]
    perms += [sr.permute(idx, 64, sr.instance_key(SEED, 12, dr.POOL_J)), sr.permute(idx, 64, sr.instance_key(SEED + 1, 11, dr.POOL_J))]
    for a in range(len(perms)):
        for b in range(a + 1, len(perms)):
            assert (perms[a] == perms[b]).mean() < 0.25, (a, b)
    rows = dr.pool_rows(*key, 64)
    assert np.array_equal(rows[0], perms[1][:16]) and np.array_equal(rows[1], sr.permute(np.arange(4), 16, sr.instance_key(*key, dr.POOL_J | 1)))


def test_dzi_rule_is_the_host_arithmetic(monkeypatch):
    """the header's operation list against pc_sample.dzi_windows + roi_transform fed the restated uniforms in the reference's
    order (random_sample(), then random_sample(2)): equal bits, the max(H, W) clip and one-pixel boxes included"""
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    FLAGS.reset()
    H, W, O = 96, 128, 64
    boxes = np.array([[10, 20, 50, 70], [0, 0, 128, 96], [3, 5, 4, 6], [60, 40, 61, 90], [100, 80, 127, 95], [5, 5, 120, 6]])
    u = dr.dzi_uniforms(SEED, 9, len(boxes))
    feed = iter([v for row in u for v in (row[0], row[1:].copy())])
    monkeypatch.setattr(np.random, "random_sample", lambda size=None: next(feed))
    centers, scales = pc_sample.dzi_windows(boxes, H, W)
    want = pc_sample.roi_transform(centers, scales, O)
    got = dr.dzi_xf(boxes, SEED, 9, H, W, O, FLAGS.DZI_PAD_SCALE, FLAGS.DZI_SCALE_RATIO, FLAGS.DZI_SHIFT_RATIO)
    assert (scales == max(H, W)).any() and (scales < max(H, W)).any()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_flag_and_resolve_draws():
    from hs_pose_amd import pc_sample
    from hs_pose_amd.config import FLAGS
    FLAGS.reset()
    assert FLAGS.step_draws == "host"
    assert pc_sample.resolve_draws(None, "cpu") is None and pc_sample.resolve_draws("host", "cpu") is None
    s = pc_sample.DeviceSampler(5, "cpu")
    assert pc_sample.resolve_draws(s, "cpu") is s
    FLAGS.step_draws = "device"
    try:
        assert pc_sample.resolve_draws(None, "cpu") is pc_sample.default_sampler("cpu")
        assert pc_sample.resolve_draws("host", "cpu") is None
        with pc_sample.draw_scope(None, "cpu") as scope:                         # (the kernels are GPU-only: a CPU forward draws on the host)
            assert scope is None and pc_sample.active_draws() is None
    finally:
        FLAGS.reset()
    with pytest.raises(ValueError):
        pc_sample.resolve_draws("gpu", "cpu")
    assert pc_sample.active_draws() is None


def test_entry_points_validate_arguments_without_gpu():
    from hs_pose_amd._lib import lib
    L = lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    # hsp_pool_rows_draw(key, n0, rate, levels, rows, stream)
    ok = [one, 1028, 4, 2, one, null]
    assert all(L.hsp_pool_rows_draw(*[null if i == k else a for i, a in enumerate(ok)]) == -1 for k in (0, 4))
    for i, v in ((1, 0), (1, -4), (2, 0), (2, -1), (3, 0), (3, 3), (1, 3), (1, 15), (2, 2000)):   # n0, rate, levels, an m of 0
        a = list(ok)
        a[i] = v
        assert L.hsp_pool_rows_draw(*a) == -1, (i, v)
    # hsp_pose_augment_keyed(12 tensors, key, aug_pc_r, B, N, M, 4 probabilities, 4 outputs, stream)
    ok = [one] * 13 + [0.2, 2, 8, 4, 0.3, 0.3, 0.3, 0.2] + [one] * 4 + [null]
    for k in list(range(13)) + [21, 22, 23, 24]:
        assert L.hsp_pose_augment_keyed(*[null if i == k else a for i, a in enumerate(ok)]) == -1, k
    for i, v in ((14, 0), (15, 0), (16, 0), (14, -1), (14, 2 ** 24 + 1), (15, 2 ** 29 + 1)):      # B, N, M
        a = list(ok)
        a[i] = v
        assert L.hsp_pose_augment_keyed(*a) == -1, (i, v)
    # hsp_dzi_windows(bboxes, key, M, H, W, out_size, pad_scale, scale_ratio, shift_ratio, xf, stream)
    ok = [one, one, 5, 96, 128, 64, 1.5, 0.25, 0.25, one, null]
    for k in (0, 1, 9):
        assert L.hsp_dzi_windows(*[null if i == k else a for i, a in enumerate(ok)]) == -1, k
    for i, v in ((2, 0), (2, 65536), (3, 0), (4, -1), (5, 0), (5, 46341), (6, 0.0), (6, float("nan")), (6, float("inf")),
                 (7, -0.1), (7, 1.0), (7, float("nan")), (8, -1.0), (8, float("inf")), (8, float("nan"))):
        a = list(ok)
        a[i] = v
        assert L.hsp_dzi_windows(*a) == -1, (i, v)
