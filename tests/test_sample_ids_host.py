"""CPU: the device sampler's construction (include/hsp.h: hsp_sample_ids) through its numpy restatement
(tests/_sample_ids_ref.py) -- the permutation is one, the branch rules hold, keys separate, the kept subset is uniform -- and the
host half of its surface: pc_sample.DeviceSampler's state, config.FLAGS.pc_sampler, argument checks that launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

import _sample_ids_ref as sr


@pytest.mark.parametrize("c", [1, 2, 3, 5, 16, 17, 257, 1028, 4096, 4097, 65536])
def test_permutation_is_a_bijection(c):
    for seed, call, j in ((0, 0, 0), (12345, 7, 3)):
        p = sr.permute(np.arange(c), c, sr.instance_key(seed, call, j))
        assert p.min() == 0 and p.max() == c - 1 and np.array_equal(np.sort(p), np.arange(c)), (c, seed, call, j)


def test_width_is_the_smallest_even_one():
    for c, half in ((1, 1), (2, 1), (4, 1), (5, 2), (16, 2), (17, 3), (64, 3), (65, 4), (4000, 6), (4097, 7), (65536, 8),
                    (65537, 9), (2 ** 31 - 1, 16)):
        assert sr.half_bits(c) == half
        assert 2 ** (2 * half) >= c and (half == 1 or 2 ** (2 * half - 2) < c)


def test_branches():
    from hs_pose_amd.pc_sample import sample_point_ids
    S = 40
    counts = np.array([0, 1, 2, 7, 39, 40, 41, 500])
    state = np.random.get_state()[1].copy()
    # short_mode 0, min_pts 2: 0 and 1 rejected; 2..39 tile exactly like _sample_points' short branch; 40 identity; the rest permuted
    ch, st = sr.sample_ids(counts, S, 5, 0, 2)
    assert st.tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and (ch[:2] == -1).all()
    for j in (2, 3, 4, 5):
        assert np.array_equal(ch[j], sample_point_ids(int(counts[j]), S)), j
    assert np.array_equal(state, np.random.get_state()[1])                     # (those branches draw nothing)
    assert np.array_equal(ch[5], np.arange(S))
    for j in (6, 7):
        assert len(set(ch[j].tolist())) == S and ch[j].min() >= 0 and ch[j].max() < counts[j]
        assert not np.array_equal(ch[j], np.arange(S))
    # short_mode 1: short rows draw WITH replacement inside [0, c), c == S is permuted, long rows as before
    ch1, st1 = sr.sample_ids(counts, S, 5, 0, 2, short_mode=1)
    assert st1.tolist() == st.tolist() and (ch1[:2] == -1).all()
    for j in (2, 3, 4):
        assert ch1[j].min() >= 0 and ch1[j].max() < counts[j]
        assert not np.array_equal(ch1[j], np.arange(S) % counts[j])
    assert len(set(ch1[4].tolist())) < S                                        # 40 draws from 39
    assert sorted(ch1[5].tolist()) == list(range(S)) and not np.array_equal(ch1[5], np.arange(S))
    assert np.array_equal(ch1[6:], ch[6:])
    # min_pts 1 accepts a count of 1 (every row 0) and still rejects 0; min_pts 50 rejects up to 41
    ch, st = sr.sample_ids(counts, S, 5, 0, 1)
    assert st.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and (ch[0] == -1).all() and (ch[1] == 0).all()
    assert sr.sample_ids(counts, S, 5, 0, 50)[1].tolist() == [1, 1, 1, 1, 1, 1, 1, 0]
    # a count of 0 is a row of -1 even where min_pts lets it through
    ch, st = sr.sample_ids(counts, S, 5, 0, 0)
    assert st[0] == 0 and (ch[0] == -1).all()
    # pairs: bit 1 from the second count, alone or with bit 0
    pairs = np.array([[100, 0], [100, 1], [100, 2], [1, 1], [1, 5]])
    ch, st = sr.sample_ids(pairs, S, 5, 0, 2, min_depth_pts=2)
    assert st.tolist() == [2, 2, 0, 3, 1] and (ch[[0, 1, 3, 4]] == -1).all() and (ch[2] >= 0).all()
    assert sr.sample_ids(pairs, S, 5, 0, 2, min_depth_pts=0)[1].tolist() == [0, 0, 0, 1, 1]
    assert sr.sample_ids(pairs[:, 0], S, 5, 0, 2, min_depth_pts=2)[1].tolist() == [0, 0, 0, 1, 1]   # single counts: no bit 1


def test_keys_separate_and_repeat():
    S = 64
    counts = np.array([3000, 3000, 30, 30])
    base, _ = sr.sample_ids(counts, S, 11, 4, 2, short_mode=1)
    again, _ = sr.sample_ids(counts, S, 11, 4, 2, short_mode=1)
    assert np.array_equal(base, again)
    assert not np.array_equal(base[0], base[1]) and not np.array_equal(base[2], base[3])          # across j
    for seed, call in ((11, 5), (12, 4), (11, 4 + 2 ** 32), (11 + 2 ** 32, 4), (2 ** 64 - 1, 2 ** 64 - 1)):
        other, _ = sr.sample_ids(counts, S, seed, call, 2, short_mode=1)
        for j in range(4):
            assert not np.array_equal(base[j], other[j]), (seed, call, j)


def test_kept_subset_is_uniform():
    """c = 4000, S = 1028, T = 4000 consecutive call counters of one seed.  Inclusion count per index standardised by
    sqrt(T p (1 - p)), p = S / c: variance within [0.9, 1.1] (an ideal sampler's spread is +-0.022) and max |z| < 5.5 (an ideal
    one exceeds it once in about 7000 such tests); adjacent index pairs kept together within 2 % of T S (S - 1) / c."""
    c, S, T = 4000, 1028, 4000
    hits = np.zeros(c, dtype=np.int64)
    pairs = 0
    xs = np.arange(S)
    for call in range(T):
        kept = np.zeros(c + 1, dtype=bool)
        kept[sr.permute(xs, c, sr.instance_key(2024, call, 0))] = True
        hits += kept[:c]
        pairs += int((kept[:-1] & kept[1:]).sum())
    p = S / c
    z = (hits - T * p) / np.sqrt(T * p * (1 - p))
    expect_pairs = T * S * (S - 1) / c
    print(f"variance {z.var():.4f}  max |z| {np.abs(z).max():.3f}  adjacent pairs {pairs} vs {expect_pairs:.0f} "
          f"({100 * (pairs / expect_pairs - 1):+.3f} %)")
    assert 0.9 <= z.var() <= 1.1
    assert np.abs(z).max() < 5.5
    assert abs(pairs / expect_pairs - 1) < 0.02


def test_sampler_state_reproduces_the_next_draws():
    from hs_pose_amd.pc_sample import DeviceSampler
    s = DeviceSampler(2 ** 64 - 3, "cpu")                                       # (a host-side key: the words can be read back)
    assert s.get_state() == (2 ** 64 - 3, 0)

    def draw():
        seed, call = (int(v) & (2 ** 64 - 1) for v in s.advance().tolist())
        return (seed, call), sr.sample_ids(np.array([5000]), 32, seed, call, 2)[0]

    (k0, a0), (k1, a1) = draw(), draw()
    assert k0 == (2 ** 64 - 3, 0) and k1 == (2 ** 64 - 3, 1) and not np.array_equal(a0, a1)
    state = s.get_state()
    assert state == (2 ** 64 - 3, 2)
    (_, a2), (_, a3) = draw(), draw()
    s.set_state(state)
    (k2, b2), (_, b3) = draw(), draw()
    assert k2 == (2 ** 64 - 3, 2) and np.array_equal(a2, b2) and np.array_equal(a3, b3)
    s.manual_seed(9)
    assert s.get_state() == (9, 0) and draw()[0] == (9, 0)


def test_default_surface(flags):
    from hs_pose_amd import pc_sample
    from hs_pose_amd.frame import FramePipeline
    assert flags.pc_sampler == "host"
    cpu = torch.device("cpu")
    assert pc_sample.resolve_sampler(None, cpu) is None and pc_sample.resolve_sampler("host", cpu) is None
    before = np.random.get_state()[1].copy()
    pc_sample._default_samplers.clear()                                         # (made on first use, from the seed of that moment)
    flags.pc_sampler = "device"
    d = pc_sample.resolve_sampler(None, cpu)
    assert isinstance(d, pc_sample.DeviceSampler) and d is pc_sample.resolve_sampler("device", cpu)
    assert d.seed == torch.initial_seed() & (2 ** 64 - 1)
    assert np.array_equal(before, np.random.get_state()[1])                     # not seeded from numpy's generator
    own = pc_sample.DeviceSampler(1, cpu)
    assert pc_sample.resolve_sampler(own, cpu) is own
    flags.pc_sampler = "host"
    assert pc_sample.resolve_sampler(None, cpu) is None
    with pytest.raises(ValueError):
        pc_sample.resolve_sampler("numpy", cpu)
    # the host sampler cannot be captured or left unsynchronised: said before anything is launched
    for kw in (dict(one_graph=True), dict(sync=False)):
        with pytest.raises(ValueError, match="device sampler"):
            FramePipeline(None, None, None, **kw)(torch.zeros(4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8),
                                                  np.array([[0, 0, 2, 2]]), np.array([1]), np.eye(3))


def test_ops_reject_cpu_tensors_and_bad_sizes():
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspError
    count, key = torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(HspError, match="GPU tensor"):
        ops.sample_ids(count, 8, key, 2)
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda:0")
    count, key = count.to(dev), key.to(dev)
    for bad in (dict(count=count.long()), dict(count=count.reshape(3, 1)), dict(count=count[:0]), dict(key=key.int()),
                dict(key=key[:1]), dict(S=0), dict(short_mode=2), dict(key=key.cpu()),
                dict(count=torch.zeros(3, 3, dtype=torch.int32, device=dev))):
        args = dict(count=count, S=8, key=key, min_pts=2)
        args.update(bad)
        with pytest.raises(HspError):
            ops.sample_ids(**args)


def test_entry_point_validates_arguments_without_gpu():
    from hs_pose_amd._lib import lib
    fn = lib().hsp_sample_ids
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    ok = [one, 1, 4, 1028, 2, 0, 0, one, one, one, null]
    for i in (0, 7, 8, 9):                                                       # count, key, choose, status
        a = list(ok)
        a[i] = null
        assert fn(*a) == -1, i
    for i, v in ((1, 0), (1, 3), (2, 0), (2, -1), (2, 65536), (3, 0), (3, -5), (6, 2), (6, -1)):   # stride, n, S, short_mode
        a = list(ok)
        a[i] = v
        assert fn(*a) == -1, (i, v)
    a = list(ok)
    a[2], a[3] = 65535, 40000                                                    # n * S >= 2^31
    assert fn(*a) == -1
