"""Inputs of the augmentation / head-split reference suites, shared by the host tests (tests/test_aug_heads_reference_host.py) and
the GPU tests (tests/test_gpu_augment_reference.py, tests/test_gpu_head_split_reference.py): numpy fp32 arrays from a seeded
RandomState, so both sides see the same bits."""
import itertools

import numpy as np

F32 = np.float32
P_STAGES = (0.3, 0.45, 0.6, 0.75)                 # p_bb, p_rt, p_bc, p_pc: four different values
AUG_PC_R = F32(0.2)
LOGITS = [0.0] + [s * v for v in (1e-3, 1.0, 17.0, 30.0, 87.5, 89.0, 104.0, float("inf")) for s in (1.0, -1.0)] + [float("nan")]


def _rotations(rng, B, spread=None):
    """(B, 3, 3) proper rotations (QR of a random matrix, or of I + spread * noise for a small one), rounded to fp32"""
    a = rng.rand(B, 3, 3) - 0.5
    q, r = np.linalg.qr(a if spread is None else np.eye(3) + spread * a)
    q = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[:, None, :]
    q = q * np.sign(np.linalg.det(q))[:, None, None]
    return q.astype(F32)


def augment_inputs(seed, B, N, M, obj, sym0, near=None):
    """B clouds of N object-frame points inside the object's box, carried to the camera frame; half of them (``near`` false) at
    0.8 m depth, half with |t| < 5 cm so that |t| does not dominate the magnitudes; sizes s + mean_shape >= 0.105 on every axis; a
    model cloud of M points in NOCS units (the box / nocs_scale).  -> dict of fp32 arrays (tests/_aug_heads_ref.INPUT_KEYS) plus
    ``noise`` (B, N, 3) = ``noise_raw`` * 0.2 in fp32."""
    rng = np.random.RandomState(seed)
    r = lambda *sh: rng.rand(*sh)
    near = (np.arange(B) % 2 == 1) if near is None else np.asarray(near)
    R = _rotations(rng, B)
    mean_shape = (0.12 + 0.03 * r(B, 3)).astype(F32)
    s = (0.03 * (r(B, 3) - 0.5)).astype(F32)
    size = s.astype(np.float64) + mean_shape
    t = np.where(near[:, None], 0.05 * (r(B, 3) - 0.5), 0.1 * (r(B, 3) - 0.5) + np.array([0.0, 0.0, 0.8])).astype(F32)
    obj_pts = (r(B, N, 3) - 0.5) * size[:, None]
    PC = (np.einsum("bnj,bij->bni", obj_pts, R.astype(np.float64)) + t[:, None]).astype(F32)
    nocs_scale = (0.2 + 0.2 * r(B)).astype(F32)
    model = ((r(B, M, 3) - 0.5) * size[:, None] / nocs_scale[:, None, None]).astype(F32)
    sym = np.zeros((B, 4), F32)
    sym[:, 0] = sym0
    noise_raw = r(B, N, 3).astype(F32)
    return dict(PC=PC, gt_R=R, gt_t=t, gt_s=s, mean_shape=mean_shape, sym=sym, aug_bb=(0.8 + 0.4 * r(B, 3)).astype(F32),
                aug_rt_t=(0.02 * (r(B, 3) - 0.5)).astype(F32), aug_rt_r=_rotations(rng, B, 0.05), model_point=model,
                nocs_scale=nocs_scale, obj_id=np.asarray(obj, F32).reshape(B), noise_raw=noise_raw,
                noise=(noise_raw * AUG_PC_R).astype(F32), ey=r(2, B).astype(F32))


def forced_draws(fire, p, ey):
    """(6, B) fp32 draws that make stage q fire on cloud b iff fire[q][b]: u = p / 2 fires, u = (1 + p) / 2 does not"""
    u = lambda f, q: np.where(f, q / 2.0, (1.0 + q) / 2.0)
    fire = np.asarray(fire, bool)
    return np.stack([u(fire[0], p[0]), u(fire[1], p[1]), u(fire[2], p[2]), ey[0], ey[1], u(fire[3], p[3])]).astype(F32)


def case_all_combinations(N=257, M=1024):
    """96 clouds: every one of the 16 stage combinations x sym[:, 0] in {0, 1} x category in {1, 5, 2}"""
    combos = list(itertools.product(range(16), (0.0, 1.0), (1.0, 5.0, 2.0)))
    B = len(combos)
    fire = np.array([[(c >> q) & 1 for c, _, _ in combos] for q in range(4)], bool)
    # the depth follows the parity of (stages fired + symmetry + category index): 48 clouds each, and each depth meets every
    # stage, both symmetries and every category
    near = [(bin(c).count("1") + int(s) + i % 3) % 2 == 1 for i, (c, s, _) in enumerate(combos)]
    inp = augment_inputs(7001, B, N, M, [o for _, _, o in combos], [s for _, s, _ in combos], near=near)
    return inp, forced_draws(fire, P_STAGES, inp["ey"]), P_STAGES


def case_all_fire(N, M, B=12):
    """every stage fires on every cloud: bowls and mugs, both symmetries"""
    inp = augment_inputs(7100 + 7 * N + M, B, N, M, [1.0, 5.0] * (B // 2), [0.0, 0.0, 1.0, 1.0] * (B // 4))
    return inp, forced_draws(np.ones((4, B), bool), P_STAGES, inp["ey"]), P_STAGES


def case_probability_edges(N=33, M=40, B=6):
    """-> inputs and three (draws, probabilities, fires) settings: a draw equal to its probability (no stage fires), p = 0 with
    u = 0 (none fires), p = 1 with u = nextafter(1, 0) (all fire).  Bowls and mugs, so that the taper may fire."""
    inp = augment_inputs(7200, B, N, M, [1.0, 5.0] * (B // 2), [0.0, 1.0, 1.0] * (B // 3))
    one = np.ones(B, F32)
    settings = []
    for p, u, fires in ((P_STAGES, [F32(q) for q in P_STAGES], False), ((0.0,) * 4, [F32(0.0)] * 4, False),
                        ((1.0,) * 4, [np.nextafter(F32(1.0), F32(0.0))] * 4, True)):
        draws = np.stack([u[0] * one, u[1] * one, u[2] * one, inp["ey"][0], inp["ey"][1], u[3] * one]).astype(F32)
        settings.append((draws, p, fires))
    return inp, settings


PLANT_AT = lambda M: (0, 255, 256, M - 1)


def case_planted_extremes(N=5, M=1024):
    """24 clouds: cloud (e, i) has the model's extreme e (min / max of x, y, z) planted at index i of (0, 255, 256, M - 1) -- the
    first lane, the last lane, the second trip of a 256-wide loop and the last element -- at eight times the box, so that no other
    point can take its place after the taper (the model is in NOCS units and s_y in metres, as in the reference, so a factor reaches
    about 2.4 in size; the planted point of an x or z extreme sits at y = 0, where the factor is at least 0.8).  The taper fires on all, the box scaling on every other cloud.
    -> inputs, draws, probabilities, [(axis, is_max, index)] per cloud."""
    plants = [(ax, mx, i) for ax in range(3) for mx in (False, True) for i in PLANT_AT(M)]
    B = len(plants)
    inp = augment_inputs(7300, B, N, M, [1.0, 5.0] * (B // 2), [0.0, 1.0, 1.0] * (B // 3))
    for b, (ax, mx, i) in enumerate(plants):
        half = np.abs(inp["model_point"][b, :, ax]).max()
        inp["model_point"][b, i, ax] = F32((8.0 if mx else -8.0) * half)
        if ax != 1:
            inp["model_point"][b, i, 1] = 0.0                    # mid-height: its own factor is (ey_up + ey_down) / 2 >= 0.8
    fire = np.ones((4, B), bool)
    fire[0] = np.arange(B) % 2 == 0
    fire[1] = False
    fire[3] = False
    return inp, forced_draws(fire, P_STAGES, inp["ey"]), P_STAGES, plants


# ---- head splits -------------------------------------------------------------------------------------------------------------------

def face_generic(R, seed=7400):
    """-> face (R, 30) fp32 of unit-scale values and the three upstream gradients (R, 6, 3), (R, 6), (R, 6)"""
    rng = np.random.RandomState(seed + R % 1000)
    g = lambda *sh: (2.0 * rng.rand(*sh) - 1.0).astype(F32)
    face = g(R, 30)
    face[:, 24:] *= F32(6.0)                                     # logits over the sigmoid's bend
    return face, g(R, 6, 3), g(R, 6), g(R, 6)


DECADES = [10.0 ** e for e in range(-12, 13)]


def face_edges(seed=7500):
    """one row per decade of |v| from 1e-12 to 1e12 (all six normals of the row at that length), the upstream gradient of faces
    0-1 parallel to the normal, of faces 2-3 antiparallel, of faces 4-5 orthogonal; the logits cycle through LOGITS, so every one of
    them occurs several times; one last row of unit normals whose face 0 is the zero vector.
    -> face (26, 30), g_nrm (26, 6, 3), g_dis, g_conf (26, 6), special (26, 6) bool: a non-finite logit or a zero normal there"""
    rng = np.random.RandomState(seed)
    Rr = len(DECADES) + 1
    lens = np.array(DECADES + [1.0])
    d = rng.randn(Rr, 6, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    v = (d * lens[:, None, None]).astype(F32)
    o = np.cross(d, rng.randn(Rr, 6, 3))
    o /= np.linalg.norm(o, axis=-1, keepdims=True)
    scale = 0.5 + rng.rand(Rr, 6, 1)
    a = np.concatenate([d[:, :2], -d[:, 2:4], o[:, 4:]], axis=1) * scale
    v[-1, 0] = 0.0
    logits = np.array([LOGITS[i % len(LOGITS)] for i in range(Rr * 6)], F32).reshape(Rr, 6)
    face = np.concatenate([v.reshape(Rr, 18), (2.0 * rng.rand(Rr, 6) - 1.0).astype(F32), logits], axis=1).astype(F32)
    special_conf = ~np.isfinite(logits)
    special_nrm = np.zeros((Rr, 6), bool)
    special_nrm[-1, 0] = True
    g = lambda *sh: (2.0 * rng.rand(*sh) - 1.0).astype(F32)
    return face, a.astype(F32), g(Rr, 6), g(Rr, 6), special_nrm, special_conf


AXIS_LENGTHS = (0.0, 1e-7, 1e-6, 1e-3, 1.0, 1e3)


def axis_case(B, seed=7600):
    """h (B, 4): |v| cycles through AXIS_LENGTHS, the logit through LOGITS; g_axis (B, 3), g_conf (B,).
    -> h, g_axis, g_conf, zero (B,) bool: a zero axis row, special (B,) bool: a non-finite logit"""
    rng = np.random.RandomState(seed + B)
    d = rng.randn(B, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    lens = np.array([AXIS_LENGTHS[b % len(AXIS_LENGTHS)] for b in range(B)])
    # (the two cycles have lengths 6 and 18: shift the logit by one every six rows so that each length meets each logit)
    logits = np.array([LOGITS[(b + b // 6) % len(LOGITS)] for b in range(B)], F32)
    h = np.concatenate([logits[:, None], (d * lens[:, None]).astype(F32)], axis=1).astype(F32)
    g = lambda *sh: (2.0 * rng.rand(*sh) - 1.0).astype(F32)
    return h, g(B, 3), g(B), lens == 0.0, ~np.isfinite(logits)
