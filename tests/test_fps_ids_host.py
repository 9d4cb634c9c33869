"""CPU: the farthest-point instance sampler's contract (include/hsp.h: hsp_fps_ids_*) through its numpy restatement
(tests/_fps_ids_ref.py) on hand-made cases -- the thinning is strictly increasing and stays inside the row, short counts tile,
a tiled cloud yields its distinct points first -- and the host half of its surface: pc_sample.FpsSampler and
config.FLAGS.pc_sampler = 'fps', the refusals of the front ends that keep their draws, the cap, argument checks that launch
nothing."""
import ctypes

import numpy as np
import pytest
import torch

import _fps_ids_ref as fr


def test_cap_is_the_register_kernel_s():
    from hs_pose_amd._lib import lib
    assert lib().hsp_fps_ids_cap() == 12288 == fr.CAP


@pytest.mark.parametrize("c", [fr.CAP + 1, 5 * fr.CAP + 3])
def test_thinning_is_strictly_increasing_and_inside_the_row(c):
    g = fr.candidate_entries(c)
    assert len(g) == fr.CAP and g[0] == 0 and g[-1] < c
    assert (np.diff(g) >= 1).all()
    # the rule in the header's own words, uint64 arithmetic: no overflow up to c = 2^31 - 1
    t = np.arange(fr.CAP, dtype=np.uint64)
    assert np.array_equal((t * np.uint64(c)) // np.uint64(fr.CAP), g.astype(np.uint64))
    big = 2 ** 31 - 1
    assert fr.g_of(fr.CAP - 1, big) == ((fr.CAP - 1) * big) // fr.CAP < big and (fr.CAP - 1) * big < 2 ** 64


def test_no_thinning_up_to_the_cap():
    for c in (1, 1028, fr.CAP - 1, fr.CAP):
        assert np.array_equal(fr.candidate_entries(c), np.arange(c))


def _flat_frame(H=8, W=40):
    """every pixel valid, depth varying so that no two pixels share coordinates"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (500 + 3 * xx + 7 * yy).astype(np.float32)


K = np.array([[50.0, 0.0, 20.0], [0.0, 60.0, 4.0], [0.0, 0.0, 1.0]])


def test_status_and_tiling():
    depth = _flat_frame()
    S = 16
    src = np.tile(np.arange(40), (6, 1))
    count = np.array([[0, 9], [3, 9], [7, 9], [16, 16], [30, 1], [30, 30]])
    ch, st = fr.fps_ids(depth, K, src, count, S, min_pts=5, min_depth_pts=2)
    assert st.tolist() == [1, 1, 0, 0, 2, 0]
    assert (ch[0] == -1).all() and (ch[1] == -1).all() and (ch[4] == -1).all()
    assert np.array_equal(ch[2], np.arange(S) % 7)                                # c < S: tiled
    assert np.array_equal(ch[3], np.arange(S))                                    # c == S: identity
    assert ch[5, 0] == 0 and len(set(ch[5].tolist())) == S and ch[5].max() < 30   # c > S: S different candidates from 0 on
    # a count of 0 that min_pts lets through is still a row of -1
    ch, st = fr.fps_ids(depth, K, src[:1], count[:1], S, min_pts=0, min_depth_pts=2)
    assert st.tolist() == [0] and (ch == -1).all()


def test_a_tiled_cloud_yields_its_distinct_points_first():
    """5 distinct points, each 4 times (an up-sampled crop), S = 8: the 5 distinct ones, then the lowest unpicked indices"""
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [1, 1, 1]], dtype=np.float32)
    cloud = np.repeat(pts, 4, axis=0)                                             # index i holds point i // 4
    picks = fr.fps_never_repick(cloud, 8)
    assert picks[0] == 0 and sorted((picks[:5] // 4).tolist()) == [0, 1, 2, 3, 4]
    assert (picks[:5] % 4 == 0).all()                                             # the lowest index of each point
    assert picks[5:].tolist() == [1, 2, 3]                                        # all at distance 0: the lowest unpicked
    assert len(set(picks.tolist())) == 8
    # the same through the whole model: a frame whose 5 pixels are each named 4 times by src
    depth = _flat_frame()
    src = np.repeat(np.array([3, 50, 97, 200, 311]), 4)[None, :]
    ch, st = fr.fps_ids(depth, K, src, np.array([[20, 20]]), 8, min_pts=2)
    assert st.tolist() == [0] and len(set(src[0, ch[0, :5]].tolist())) == 5 and sorted(ch[0, 5:].tolist()) == ch[0, 5:].tolist()
    assert len(set(ch[0].tolist())) == 8


def test_picks_follow_the_plain_rule_where_nothing_repeats(oc):
    """on a cloud whose plain picks are all distinct the never-repick picks are the plain fp32 picks of the C oracle"""
    rng = np.random.RandomState(3)
    depth = rng.randint(400, 900, size=(24, 32)).astype(np.float32)
    pix = rng.permutation(24 * 32)[:300]
    xyz = fr.back_project(depth, K, pix)
    assert xyz.dtype == np.float32 and len(np.unique(xyz, axis=0)) == 300
    assert np.array_equal(fr.fps_never_repick(xyz, 64), oc.fps_f32(xyz[None], 64)[0])


def test_sampler_switch(flags):
    from hs_pose_amd import pc_sample
    cpu = torch.device("cpu")
    s = pc_sample.resolve_sampler("fps", cpu)
    assert isinstance(s, pc_sample.FpsSampler) and s is pc_sample.FPS and pc_sample.resolve_sampler(s, cpu) is s
    assert s.advance() is None and s.key is None and hash(s) == hash(pc_sample.FPS) and {s: 1}[pc_sample.FPS] == 1
    assert flags.pc_sampler == "host" and pc_sample.resolve_sampler(None, cpu) is None
    flags.pc_sampler = "fps"
    assert pc_sample.resolve_sampler(None, cpu) is pc_sample.FPS
    assert pc_sample.resolve_sampler("host", cpu) is None
    assert isinstance(pc_sample.resolve_sampler("device", cpu), pc_sample.DeviceSampler)
    with pytest.raises(ValueError):
        pc_sample.resolve_sampler("numpy", cpu)


def test_front_ends_that_keep_their_draws_refuse_fps(flags):
    from hs_pose_amd import pc_sample, train
    depth = torch.zeros(2, 4, 4)
    mask = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for sampler in ("fps", pc_sample.FPS):
        with pytest.raises(ValueError, match="'fps'"):
            pc_sample.train_batch_to_pcl(depth, mask, None, np.zeros((2, 2)), np.ones(2), K, sampler=sampler)
        with pytest.raises(ValueError, match="'fps'"):
            train.FrameTrainStep(None, None, {"depth": depth}, {}, 1, sampler=sampler)
    # the flag is the frame front end's: the training front end falls back to its device sampler, not to 'fps'
    flags.pc_sampler = "fps"
    with pytest.raises(ValueError, match="'fps'"):
        pc_sample.train_batch_to_pcl(depth, mask, None, np.zeros((2, 2)), np.ones(2), K, sampler=pc_sample.FPS)


def test_argument_validation_without_gpu():
    from hs_pose_amd._lib import CONSTANTS, lib
    L = lib()
    bad = CONSTANTS["ERR_BAD_ARG"]
    assert bad == -1
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    for fn in (L.hsp_fps_ids_f32, L.hsp_fps_ids_u16):
        def call(depth=one, H=96, W=128, camK=one, rows=1, src=one, stride=1024, count=one, n=3, S=64, choose=one, status=one):
            return fn(depth, H, W, camK, rows, src, stride, count, n, S, 2, 2, choose, status, null)

        for name in ("depth", "camK", "src", "count", "choose", "status"):
            assert call(**{name: null}) == bad, name
        assert call(n=0) == bad and call(n=-1) == bad and call(n=65536) == bad
        assert call(S=0) == bad and call(S=-5) == bad
        assert call(n=65535, S=32769) == bad                                    # n * S >= 2^31
        assert call(n=2, S=2 ** 30) == bad                                      # n * S == 2^31
        assert call(rows=2) == bad and call(rows=0) == bad                      # camK_rows neither 1 nor n
        assert call(H=0) == bad and call(W=0) == bad and call(H=65536, W=32768) == bad   # H * W == 2^31
        assert call(stride=0) == bad and call(stride=-1) == bad


def test_header_states_the_contract_and_table_lists_the_entries():
    import os
    from hs_pose_amd import _lib
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hsp.h")).read()
    for name in ("hsp_fps_ids_cap", "hsp_fps_ids_f32", "hsp_fps_ids_u16"):
        assert name in _lib.SIGNATURES and f"int {name}(" in txt
    assert "g(t) = (uint64(t) * c) / CAP" in txt and "A PICKED CANDIDATE IS NEVER PICKED AGAIN" in txt
    assert not [n for n in _lib.SIGNATURES if n.startswith("hsp_fps_ids") and n.endswith("_takes")]
