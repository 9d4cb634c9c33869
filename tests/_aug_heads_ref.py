"""float64 references of the training-step augmentation (hsp_pose_augment) and of the two head splits (hsp_face_split_*,
hsp_axis_conf_*), with the per-element error budget an fp32 evaluation of the same formulas may use.  Written from the text of
hs_pose_amd/augment.py, hs_pose_amd/PoseNet9D.py and the comments of include/hsp.h; they call no kernel and restate none.

The budget of an output element is
    bound = (n + 2) * 2^-24 * mag
where mag is the same expression evaluated on absolute values with every subtraction turned into an addition (the running
magnitude tests/test_gpu_gemm_rows.py calls ``mag``), and n is the number of fp32 roundings on the longest path from the inputs
to that element through the stages that fired for its cloud.  The inputs are fp32 values and carry no error; a constant of the
fp32 code enters with the value the fp32 code has (C04, C08, EPS32 below).  Contracting a product and a sum into one FMA removes
a rounding, so it only lowers n.  The "+ 2" is slack for the order of a three-term sum and for a constant that differs from ours
by an ulp (the torch composition multiplies by float32(1.2 - 0.8), one ulp below float32(1.2) - float32(0.8)).

The augmentation is numpy (host sizes); the head splits are torch float64 and run on whatever device their inputs are on.
"""
import numpy as np
import torch

U = 2.0 ** -24                                              # the unit roundoff of fp32
C04 = float(np.float32(1.2) - np.float32(0.8))              # the taper's range as the fp32 code has it (0.40000004)
C08 = float(np.float32(0.8))
EPS32 = float(np.float32(1e-6))                             # the axis guard as the fp32 code has it
TINY = 2.0 ** -126                                          # the smallest normal fp32: results below it may be flushed to zero

# fp32 roundings per stage on the longest path to each output (derived beside each stage in augment64)
N_PC = dict(bb=9, rt=4, bc=13, pc=3)
N_R = dict(rt=3)
N_T = dict(rt=4)
N_S = dict(bb=3, bc=9)

AUGMENT_MUTANTS = ("R_for_RT_box", "R_for_RT_taper", "no_sym", "sy_before_box", "model_unscaled", "t_stale_jitter",
                   "jitter_about_origin", "ey_swapped", "le_fires", "no_cat1")
FACE_MUTANTS = ("strided_normals", "no_projector")
AXIS_MUTANTS = ("eps_under_sqrt",)

INPUT_KEYS = ("PC", "gt_R", "gt_t", "gt_s", "mean_shape", "sym", "aug_bb", "aug_rt_t", "aug_rt_r", "model_point", "nocs_scale",
              "obj_id")


def _f64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def augment_fired(inputs, draws, p_bb, p_rt, p_bc, p_pc, mutant=None):
    """-> the four (B,) bool arrays: which stage applies to which cloud.  A stage fires where its uniform is strictly below its
    probability (the probability as the fp32 value the C entry receives); the taper only for bowls (1) and mugs (5)."""
    d = _f64(draws)
    obj = _f64(inputs["obj_id"]).reshape(-1)
    p = [float(np.float32(v)) for v in (p_bb, p_rt, p_bc, p_pc)]
    lt = (lambda u, q: u <= q) if mutant == "le_fires" else (lambda u, q: u < q)
    cat = (obj == 5.0) if mutant == "no_cat1" else ((obj == 5.0) | (obj == 1.0))
    return lt(d[0], p[0]), lt(d[1], p[1]), lt(d[2], p[2]) & cat, lt(d[5], p[3])


def augment64(inputs, draws, noise, p_bb, p_rt, p_bc, p_pc, mutant=None):
    """HSPose.data_augment in float64 on given draws.  inputs: the twelve arrays of INPUT_KEYS; draws (6, B): u_bb, u_rt, u_bc, ey_up,
    ey_down, u_pc; noise (B, N, 3): the jitter factors (rand * aug_pc_r, already multiplied).
    -> (PC, R, t, s), (magPC, magR, magt, mags).  ``mutant`` names one deliberate mistake (AUGMENT_MUTANTS): the host suite uses
    them to show that the bound tells a wrong formula from rounding."""
    PC, R, t, s, ms, sym, abb, at, ar, mp, ns, _ = [_f64(inputs[k]) for k in INPUT_KEYS]
    B = PC.shape[0]
    R, ar, sym, ns = R.reshape(B, 3, 3), ar.reshape(B, 3, 3), sym.reshape(B, -1), ns.reshape(B)
    d, noise = _f64(draws), _f64(noise)
    f_bb, f_rt, f_bc, f_pc = augment_fired(inputs, draws, p_bb, p_rt, p_bc, p_pc, mutant)
    PCm, Rm, tm, sm, mpm = np.abs(PC), np.abs(R), np.abs(t), np.abs(s), np.abs(mp)
    s_in, sm_in = s, sm
    w3 = lambda f: f[:, None]                                   # (B,) -> per-component
    w33 = lambda f: f[:, None, None]                            # (B,) -> per-point / per-matrix element

    def to_object(p, pm, R, Rm, t, tm, swap):
        """R^T (p - t) per point: 1 (difference) + 1 (product) + 2 (two sums) = 4 roundings"""
        dd, ddm = p - t[:, None], pm + tm[:, None]
        if swap:                                                # the mistake: R where R^T belongs
            return np.einsum("bji,bni->bnj", R, dd), np.einsum("bji,bni->bnj", Rm, ddm)
        return np.einsum("bni,bij->bnj", dd, R), np.einsum("bni,bij->bnj", ddm, Rm)

    def to_camera(o, om, R, Rm, t, tm):
        """R o + t per point: 1 (product) + 2 (sums) + 1 (+ t) = 4 roundings"""
        return np.einsum("bnj,bij->bni", o, R) + t[:, None], np.einsum("bnj,bij->bni", om, Rm) + tm[:, None]

    # ---- 1. box scaling in the object frame; x and z share (a0 + a2) / 2 under rotational symmetry (sym[:, 0] == 1).
    #      k: 1 rounding (the sum; the halving is exact).  PC: 4 (to the object frame) + 1 (* k) + 4 (back) = 9.
    #      s: (s + ms) 1, * k 1, - ms 1 = 3.  The model cloud: * k, 1 on top of k's 1 = 2 (never the longest path later).
    k = abb if mutant == "no_sym" else np.where(w3(sym[:, 0] == 1.0), (abb + abb[:, ::-1]) / 2.0, abb)
    km = np.abs(k)
    o, om = to_object(PC, PCm, R, Rm, t, tm, mutant == "R_for_RT_box")
    p1, p1m = to_camera(o * k[:, None], om * km[:, None], R, Rm, t, tm)
    PC, PCm = np.where(w33(f_bb), p1, PC), np.where(w33(f_bb), p1m, PCm)
    s, sm = np.where(w3(f_bb), (s + ms) * k - ms, s), np.where(w3(f_bb), (sm + np.abs(ms)) * km + np.abs(ms), sm)
    if mutant != "model_unscaled":
        mp, mpm = np.where(w33(f_bb), mp * k[:, None], mp), np.where(w33(f_bb), mpm * km[:, None], mpm)

    # ---- 2. rigid perturbation: shift by aug_rt_t, rotate everything by aug_rt_r about the camera origin.
    #      PC: (p + at) 1, product 1, two sums 2 = 4.  R: product 1, two sums 2 = 3.  t: (t + at) 1, product 1, two sums 2 = 4.
    arm, atm = np.abs(ar), np.abs(at)
    p2, p2m = np.einsum("bnj,bij->bni", PC + at[:, None], ar), np.einsum("bnj,bij->bni", PCm + atm[:, None], arm)
    R2, R2m = np.einsum("bij,bjk->bik", ar, R), np.einsum("bij,bjk->bik", arm, Rm)
    t2, t2m = np.einsum("bij,bj->bi", ar, t + at), np.einsum("bij,bj->bi", arm, tm + atm)
    t_before_rt, tm_before_rt = t, tm
    PC, PCm = np.where(w33(f_rt), p2, PC), np.where(w33(f_rt), p2m, PCm)
    R, Rm = np.where(w33(f_rt), R2, R), np.where(w33(f_rt), R2m, Rm)
    t, tm = np.where(w3(f_rt), t2, t), np.where(w3(f_rt), t2m, tm)

    # ---- 3. box-cage taper (bowls and mugs): x and z scaled by f(y), linear in y from ey_down at the bottom (y = -s_y / 2) to ey_up
    #      at the top; s_y is the y size AFTER the box scaling; the new size is the extent of the tapered (scaled) model * nocs_scale.
    #      ey: u * C04 1, + C08 1 = 2 (never the longest path).  s_y = s + ms: 1 on top of s.
    #      f: (y + s_y / 2) 1, / s_y 1, * (ey_up - ey_down) 1, + ey_down 1 = 4 on top of y (a point: 4 roundings deep by then, deeper
    #      than s_y) or, for the model, on top of s_y.
    #      PC: 4 (to the object frame) + 4 (f) + 1 (x * f) + 4 (back) = 13.
    #      s: s_y 1, f 4, x * f 1, max - min 1, * nocs_scale 1, - ms 1 = 9 on top of s.
    up, dn = d[3][:, None] * C04 + C08, d[4][:, None] * C04 + C08
    if mutant == "ey_swapped":
        up, dn = dn, up
    s_y, s_ym = (s + ms)[:, 1:2], (sm + np.abs(ms))[:, 1:2]
    if mutant == "sy_before_box":
        s_y, s_ym = (s_in + ms)[:, 1:2], (sm_in + np.abs(ms))[:, 1:2]

    def taper(q, qm):
        f = (q[..., 1] + s_y / 2.0) / s_y * (up - dn) + dn
        fm = (qm[..., 1] + s_ym / 2.0) / np.abs(s_y) * (up + dn) + dn
        return (np.stack([q[..., 0] * f, q[..., 1], q[..., 2] * f], axis=-1),
                np.stack([qm[..., 0] * fm, qm[..., 1], qm[..., 2] * fm], axis=-1))

    with np.errstate(all="ignore"):                             # (clouds the taper does not fire on may divide by a zero size)
        o, om = to_object(PC, PCm, R, Rm, t, tm, mutant == "R_for_RT_taper")
        o, om = taper(o, om)
        p3, p3m = to_camera(o, om, R, Rm, t, tm)
        m3, m3m = taper(mp, mpm)
        # max and min are 1-Lipschitz in the largest element error, so their magnitude is the largest element magnitude
        s3 = (m3.max(axis=1) - m3.min(axis=1)) * ns[:, None] - ms
        s3m = 2.0 * m3m.max(axis=1) * np.abs(ns)[:, None] + np.abs(ms)
    PC, PCm = np.where(w33(f_bc), p3, PC), np.where(w33(f_bc), p3m, PCm)
    s, sm = np.where(w3(f_bc), s3, s), np.where(w3(f_bc), s3m, sm)

    # ---- 4. radial jitter about the (perturbed) object centre: p + noise * (p - t).  (p - t) 1, product 1, sum 1 = 3.
    c, cm = t, tm
    if mutant == "t_stale_jitter":
        c, cm = t_before_rt, tm_before_rt
    if mutant == "jitter_about_origin":
        c, cm = np.zeros_like(t), np.zeros_like(tm)
    p4, p4m = PC + noise * (PC - c[:, None]), PCm + np.abs(noise) * (PCm + cm[:, None])
    PC, PCm = np.where(w33(f_pc), p4, PC), np.where(w33(f_pc), p4m, PCm)
    return (PC, R, t, s), (PCm, Rm, tm, sm)


def augment_roundings(fired):
    """-> per-cloud n of (PC, R, t, s) for the stages that fired"""
    f_bb, f_rt, f_bc, f_pc = [np.asarray(f).astype(np.int64) for f in fired]
    return (N_PC["bb"] * f_bb + N_PC["rt"] * f_rt + N_PC["bc"] * f_bc + N_PC["pc"] * f_pc, N_R["rt"] * f_rt, N_T["rt"] * f_rt,
            N_S["bb"] * f_bb + N_S["bc"] * f_bc)


def augment_bound(mags, fired):
    """-> the four per-element bounds (n + 2) 2^-24 mag"""
    n = augment_roundings(fired)
    return tuple((nn.reshape((-1,) + (1,) * (m.ndim - 1)) + 2) * U * m for nn, m in zip(n, mags))


# ---- the sigmoid -------------------------------------------------------------------------------------------------------------------
# A fast fp32 exponential evaluates e = exp(-x) as exp2(x * log2(e)).  The product rounds once and the constant was rounded once:
# the ARGUMENT of exp2 is off by at most 2 * 2^-24 * |x| log2(e), which moves e by the relative 2 |x| 2^-24 (d exp2(y) = ln 2 e dy and
# ln 2 * log2(e) = 1); the hardware exp2 is good to 1 ulp = 2^-23.  Together (|x| + 1) 2^-23; the compiler may split the scaling in
# two (range reduction), which at most doubles it: delta_e = 2 (|x| + 2) 2^-23 relative.
# sigma = 1 / (1 + e), d sigma / d e = -1 / (1 + e)^2, so a relative delta_e on e moves sigma by e / (1 + e)^2 delta_e
# = sigma (1 - sigma) delta_e.  The sum and the quotient round once each: 2 * 2^-24 * sigma.  A result (or an e) below 2^-126 may be
# flushed to zero, and an e that overflows gives sigma = 0 where the true sigma is below 2^-126 as well: + 2^-126.
#     bound(sigma) = sigma (1 - sigma) delta_e + 2 * 2^-24 * sigma + 2^-126
# The gradient g sigma (1 - sigma): (1 - sigma) is one more rounding on top of sigma's 2, the two products one each on the longest
# path: n = 4 with mag = |g| sigma (|1| + |sigma|).  The error of e reaches both factors: |g| (|1 - sigma| + |sigma|) * sigma (1 - sigma)
# delta_e = |g| sigma (1 - sigma) delta_e.  A flushed sigma moves the product by |g| 2^-126, a flushed product by 2^-126.
#     bound(grad) = |g| sigma (1 - sigma) delta_e + (4 + 2) 2^-24 |g| sigma (1 + sigma) + (|g| + 1) 2^-126
N_SIG_GRAD = 4


def _delta_e(x):
    return 2.0 * (x.abs() + 2.0) * 2.0 ** -23


def sigmoid_bound(x):
    x = x.double()
    s, c = torch.sigmoid(x), torch.sigmoid(-x)                  # (1 - sigma as sigma(-x): no cancellation in the tail)
    return s * c * _delta_e(x) + 2.0 * U * s + TINY


def sigmoid_grad64(x, g):
    """-> (g sigma (1 - sigma), its mag, its bound) in float64"""
    x, g = x.double(), g.double()
    s, c = torch.sigmoid(x), torch.sigmoid(-x)
    mag = g.abs() * s * (1.0 + s)
    return g * s * c, mag, g.abs() * s * c * _delta_e(x) + (N_SIG_GRAD + 2) * U * mag + (g.abs() + 1.0) * TINY


# ---- the face head's split (PoseNet9D.py:31-35) ----------------------------------------------------------------------------------------
# face (R, 30): normals = face[:, :18] as (R, 6, 3) rows / their 3-norm (no epsilon), distances = face[:, 18:24], confidences =
# sigmoid(face[:, 24:]).
#   normal: three squares 1, two sums 2, the root 1, the quotient 1: n = 5, mag = |u| (nothing is subtracted).
#   its vector-Jacobian product (I - u u^T) a / |v|: u 5, a . u: product 1 + two sums 2, u (a . u) 1, a - that 1, / |v| 1: n = 11,
#   mag = (|a| + |u| sum_i |a_i| |u_i|) / |v|.
N_FACE_NRM, N_FACE_GRAD = 5, 11


def face_split64(face, g_nrm=None, g_dis=None, g_conf=None, mutant=None):
    """face (R, 30) -> (normals (R, 6, 3), dis (R, 6), conf (R, 6)), their mags, g_face (R, 30), its mag.  Any subset of the upstream
    gradients may be None (= zero); with all three None g_face and its mag are None."""
    face = face.double()
    Rr = face.shape[0]
    if mutant == "strided_normals":                             # the mistake: face f's normal read from columns f, f + 6, f + 12
        v = face[:, :18].reshape(Rr, 3, 6).transpose(1, 2)
    else:
        v = face[:, :18].reshape(Rr, 6, 3)
    n = (v * v).sum(-1, keepdim=True).sqrt()
    u = v / n
    x = face[:, 24:30]
    outs = (u, face[:, 18:24].clone(), torch.sigmoid(x))
    mags = (u.abs(), outs[1].abs(), outs[2])
    if g_nrm is None and g_dis is None and g_conf is None:
        return outs, mags, None, None
    g = torch.zeros_like(face)
    gm = torch.zeros_like(face)
    if g_nrm is not None:
        a = g_nrm.double().reshape(Rr, 6, 3)
        gv = a / n if mutant == "no_projector" else (a - u * (a * u).sum(-1, keepdim=True)) / n
        gvm = (a.abs() + u.abs() * (a.abs() * u.abs()).sum(-1, keepdim=True)) / n
        if mutant == "strided_normals":
            g[:, :18], gm[:, :18] = gv.transpose(1, 2).reshape(Rr, 18), gvm.transpose(1, 2).reshape(Rr, 18)
        else:
            g[:, :18], gm[:, :18] = gv.reshape(Rr, 18), gvm.reshape(Rr, 18)
    if g_dis is not None:
        g[:, 18:24], gm[:, 18:24] = g_dis.double().reshape(Rr, 6), g_dis.double().reshape(Rr, 6).abs()
    if g_conf is not None:
        g[:, 24:30], gm[:, 24:30], _ = sigmoid_grad64(x, g_conf.reshape(Rr, 6))
    return outs, mags, g, gm


def face_split_bounds(face, mags, g_mag=None, g_conf=None):
    """-> (bound of normals, of dis (exactly 0: a copy), of conf, of g_face or None)"""
    face = face.double()
    x = face[:, 24:30]
    b_g = None
    if g_mag is not None:
        b_g = (N_FACE_GRAD + 2) * U * g_mag
        b_g[:, 18:24] = 0.0                                     # a copy
        b_g[:, 24:30] = sigmoid_grad64(x, g_conf.reshape(x.shape))[2] if g_conf is not None else 0.0
    return (N_FACE_NRM + 2) * U * mags[0], torch.zeros_like(mags[1]), sigmoid_bound(x), b_g


# ---- a rotation head's split (PoseNet9D.py:40-46) --------------------------------------------------------------------------------------
# h (B, 4): axis = v / (|v| + 1e-6) with v = h[:, 1:], confidence = sigmoid(h[:, 0]).
#   axis: three squares 1, two sums 2, the root 1, + eps 1, the quotient 1: n = 6, mag = |v| / d (nothing is subtracted), d = |v| + eps.
#   its vector-Jacobian product a / d - (a . v) v / (|v| d^2), the second term 0 at v = 0 (the norm's subgradient torch takes):
#   a . v: product 1 + two sums 2 = 3; |v| 4, d 5, |v| d 6, * d 7; the quotient 8, * v 9, the difference 10: n = 10,
#   mag = |a| / d + (sum_i |a_i| |v_i|) |v| / (|v| d^2).
N_AXIS, N_AXIS_GRAD = 6, 10


def axis_conf64(h, g_axis=None, g_conf=None, mutant=None):
    """h (B, 4) -> (axis (B, 3), conf (B,)), their mags, g_h (B, 4), its mag (None, None when both upstream gradients are None)"""
    h = h.double()
    v = h[:, 1:]
    n = (v * v).sum(-1, keepdim=True).sqrt()
    under = mutant == "eps_under_sqrt"                          # the mistake: sqrt(|v|^2 + eps) instead of |v| + eps
    d = ((v * v).sum(-1, keepdim=True) + EPS32).sqrt() if under else n + EPS32
    outs = (v / d, torch.sigmoid(h[:, 0]))
    mags = (v.abs() / d, outs[1])
    if g_axis is None and g_conf is None:
        return outs, mags, None, None
    g, gm = torch.zeros_like(h), torch.zeros_like(h)
    if g_axis is not None:
        a = g_axis.double()
        den = d * d * d if under else n * d * d
        nz = n > 0
        safe = torch.where(nz, den, torch.ones_like(den))
        g[:, 1:] = a / d - torch.where(nz, (a * v).sum(-1, keepdim=True) / safe, torch.zeros_like(den)) * v
        gm[:, 1:] = a.abs() / d + torch.where(nz, (a.abs() * v.abs()).sum(-1, keepdim=True) / safe, torch.zeros_like(den)) * v.abs()
    if g_conf is not None:
        g[:, 0], gm[:, 0], _ = sigmoid_grad64(h[:, 0], g_conf.reshape(-1))
    return outs, mags, g, gm


def axis_conf_bounds(h, mags, g_mag=None, g_conf=None):
    """-> (bound of axis, of conf, of g_h or None)"""
    h = h.double()
    b_g = None
    if g_mag is not None:
        b_g = (N_AXIS_GRAD + 2) * U * g_mag
        b_g[:, 0] = sigmoid_grad64(h[:, 0], g_conf.reshape(-1))[2] if g_conf is not None else 0.0
    return (N_AXIS + 2) * U * mags[0], sigmoid_bound(h[:, 0]), b_g
