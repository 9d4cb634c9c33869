"""GPU: hsp_pose_augment (csrc/losses.hip) against the float64 reference of tests/_aug_heads_ref.py on draws the test supplies (no
generator), at the loader's model size M = 1024 and at every size around the 256-wide loops, every output element within
    (n + 2) 2^-24 mag,      n = the fp32 roundings on the longest path through the stages that fired for the cloud
(tests/test_aug_heads_reference_host.py shows the bound honest -- the fp32 torch composition uses less than half of it -- and
sharp: ten wrong formulas leave it by 10x or more).

Rounding counts n per fired stage:   PC: box 9, rigid 4, taper 13, jitter 3;  R: rigid 3;  t: rigid 4;  s: box 3, taper 9.
Largest err / (2^-24 mag) over the cases of this file (recorded by the last test, not asserted: the bound is the derived n + 2):
    CPU fp32 torch composition:   PC 3.8   R 2.0   t 2.1   s 0.93
    the kernel on an MI355X:      PC 3.8   R 2.0   t 2.1   s 0.93
"""
import numpy as np
import pytest
import torch

import _aug_heads_cases as C
import _aug_heads_ref as A

pytestmark = pytest.mark.gpu

NAMES = ("PC", "R", "t", "s")
RATIOS = {k: 0.0 for k in NAMES}                 # worst measured err / (2^-24 mag), printed by the last test


def _launch(dev, inp, draws, p):
    """hsp_pose_augment on numpy inputs -> the four outputs as numpy fp32 (NaN-prefilled, so an unwritten element fails)"""
    from hs_pose_amd import ops
    B, N = inp["PC"].shape[:2]
    M = inp["model_point"].shape[1]
    up = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(shape)).to(dev)
    shapes = dict(PC=(B, N, 3), gt_R=(B, 3, 3), gt_t=(B, 3), gt_s=(B, 3), mean_shape=(B, 3), sym=(B, 4), aug_bb=(B, 3), aug_rt_t=(B, 3),
                  aug_rt_r=(B, 3, 3), model_point=(B, M, 3), nocs_scale=(B,), obj_id=(B,))
    args = [up(inp[k], shapes[k]) for k in A.INPUT_KEYS] + [up(draws, (6, B)), up(inp["noise"], (B, N, 3))]
    outs = [torch.full(s, float("nan"), dtype=torch.float32, device=dev) for s in ((B, N, 3), (B, 3, 3), (B, 3), (B, 3))]
    ops._run("hsp_pose_augment", [ops._p(a) for a in args] + [B, N, M] + [float(q) for q in p] + [ops._p(o) for o in outs] +
             [ops._stream()])
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _hold(got, inp, draws, p, label):
    """every element of the four outputs within its bound; -> (reference outputs, bounds, fired)"""
    outs, mags = A.augment64(inp, draws, inp["noise"], *p)
    fired = A.augment_fired(inp, draws, *p)
    bounds = A.augment_bound(mags, fired)
    report = []
    for name, g, w, m, b in zip(NAMES, got, outs, mags, bounds):
        assert g.dtype == np.float32 and g.shape == w.shape
        err = np.abs(g.astype(np.float64) - w)
        assert not np.isnan(err).any(), (label, name)
        units = float(np.max(np.where(err > 0, err / np.maximum(A.U * m, 1e-300), 0.0)))
        RATIOS[name] = max(RATIOS[name], units)
        report.append(f"{name} {units:.2f}")
    print(f"\n  {label}: err / (2^-24 mag)  " + "  ".join(report))
    for name, g, w, b in zip(NAMES, got, outs, bounds):
        over = np.abs(g.astype(np.float64) - w) > b
        assert not over.any(), (label, name, int(over.sum()), np.argwhere(over)[:4].tolist())
    return outs, bounds, fired


def test_every_stage_combination_at_the_loaders_model_size(dev):
    """96 clouds = 16 stage combinations x rotational symmetry or not x bowl / mug / a category without taper, N = 257 (one point
    on the second trip of the point loop), M = 1024 (four trips of the model loop), four different probabilities"""
    inp, draws, p = C.case_all_combinations()
    assert inp["PC"].shape == (96, 257, 3) and inp["model_point"].shape == (96, 1024, 3) and len(set(p)) == 4
    fired = np.stack(A.augment_fired(inp, draws, *p))
    want_bits = np.stack([(np.arange(96) // 6 >> q) & 1 for q in range(4)]).astype(bool)
    want_bits[2] &= inp["obj_id"] != 2.0                       # the taper never fires on category 2, whatever its draw
    assert np.array_equal(fired, want_bits)
    combos = {(tuple(fired[:, b]), inp["sym"][b, 0], inp["obj_id"][b]) for b in range(96)}
    assert len({c[0] for c in combos if c[2] != 2.0}) == 16 and len(combos) >= 80
    size = inp["gt_s"].astype(np.float64) + inp["mean_shape"]
    assert size.min() >= 0.05
    depth = np.linalg.norm(inp["gt_t"], axis=1)
    assert (depth < 0.05).sum() == 48 and (depth > 0.7).sum() == 48
    got = _launch(dev, inp, draws, p)
    _hold(got, inp, draws, p, "combinations")
    assert np.abs(got[0] - inp["PC"]).max() > 1e-3


@pytest.mark.parametrize("N", [1, 255])
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_model_and_cloud_sizes_around_the_loop_width(dev, M, N):
    """every stage fires on 12 clouds; one model point gives a tapered extent of zero: s = -mean_shape exactly"""
    inp, draws, p = C.case_all_fire(N, M)
    got = _launch(dev, inp, draws, p)
    _, _, fired = _hold(got, inp, draws, p, f"all fire N={N} M={M}")
    assert all(f.all() for f in fired)
    if M == 1:
        assert np.array_equal(got[3], -inp["mean_shape"])


def test_probability_edges(dev):
    """a draw equal to its probability does not fire; p = 0 never fires, even on u = 0; p = 1 always fires, even on the largest
    uniform below 1; a cloud on which nothing fires comes back bit for bit, R, t and s included"""
    inp, settings = C.case_probability_edges()
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    for i, (draws, p, fires) in enumerate(settings):
        fired = A.augment_fired(inp, draws, *p)
        assert all(f.all() == fires and f.any() == fires for f in fired)
        got = _launch(dev, inp, draws, p)
        if fires:
            _hold(got, inp, draws, p, f"edges {i}")
            assert np.abs(got[0] - inp["PC"]).max() > 1e-3 and not np.array_equal(got[1], inp["gt_R"])
        else:
            for g, k in zip(got, ("PC", "gt_R", "gt_t", "gt_s")):
                assert np.array_equal(bits(g), bits(inp[k])), (i, k)


def test_taper_extent_finds_extremes_at_the_loop_edges(dev):
    """the model's extreme on one axis sits at index 0, 255, 256 or M - 1 of M = 1024 (first lane, last lane, second trip, last
    element): the new size equals the reference's within the bound (the host suite shows each planted point decides its size)"""
    inp, draws, p, plants = C.case_planted_extremes()
    assert inp["model_point"].shape[1] == 1024
    got = _launch(dev, inp, draws, p)
    outs, bounds, fired = _hold(got, inp, draws, p, "planted extremes")
    assert fired[2].all()
    for b, (ax, _, i) in enumerate(plants):
        assert abs(float(got[3][b, ax]) - outs[3][b, ax]) <= bounds[3][b, ax], (b, ax, i)


def test_report_measured_ratios():
    """not a check: prints the worst measured err / (2^-24 mag) of the cases above (the figures quoted at the head of this file)"""
    print("\n  hsp_pose_augment, worst err / (2^-24 mag): " + "  ".join(f"{k} {v:.2f}" for k, v in RATIOS.items()))
