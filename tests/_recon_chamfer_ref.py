"""fp64 restatement of the Chamfer reconstruction term 'Prop_sym_cd' (include/hsp.h: hsp_recon_chamfer_fwd / _bwd,
hsp_chamfer_bwd_ordered; hs_pose_amd/losses.py::prop_rot_loss.prop_sym_chamfer_loss), written from the formulas, not from the
kernels: the target of a cloud by its symmetry class, brute-force first-minimum searches, the term, and the gradient as a
per-row sum over given arg-min lists.  Also the batches the tests share.  numpy, float64 throughout."""
import numpy as np
import torch

# the four classes of prop_loss.py:258-276 as sym rows: 180 degrees about y | mirror in z | none | left out
SYM_Y, SYM_YX, SYM_NONE, SYM_SKIP = (1., 1., 0., 1.), (0., 1., 0., 0.), (0., 0., 0., 0.), (1., 0., 0., 0.)


def classes(sym):
    """(cls_y, cls_yx, cls_none, skip) boolean (B,) arrays"""
    s = np.asarray(sym, np.float64)
    rot = s[:, 0] == 1
    mirrors = s[:, 1:].sum(-1)
    return rot & (mirrors > 0), ~rot & (s[:, 1] == 1), ~rot & (s[:, 1] != 1), rot & (mirrors == 0)


def target64(PC, R, t, sym):
    """G (B,N,3) float64 and the per-component magnitude sum  sum_k |p_k - t_k|  (B,N) the bound on G is stated in"""
    P, R, t = (np.asarray(a, np.float64) for a in (PC, R, t))
    cls_y, cls_yx, cls_none, skip = classes(sym)
    canon = np.einsum("bnk,bkj->bnj", P - t[:, None], R)                      # R^T (p - t)
    out = np.zeros_like(P)
    for b in range(P.shape[0]):
        if cls_y[b] or cls_yx[b]:
            m = canon[b] * (np.array([-1., 1., -1.]) if cls_y[b] else np.array([1., 1., -1.]))
            out[b] = m @ R[b].T + t[b]
        elif cls_none[b]:
            out[b] = P[b]
    return out, np.abs(P - t[:, None]).sum(-1)


def search64(Q, C):
    """queries Q (n,3) against candidates C (m,3) in float64: (best distance, FIRST arg-min, runner-up distance over the other
    candidates -- inf where there is one candidate --, its first index)"""
    Q, C = np.asarray(Q, np.float64), np.asarray(C, np.float64)
    d = ((C[None] - Q[:, None]) ** 2).sum(-1)
    i = d.argmin(1)                                                           # numpy: the first occurrence
    rows = np.arange(len(Q))
    best = d[rows, i]
    d[rows, i] = np.inf
    r = d.argmin(1)
    return best, i.astype(np.int64), d[rows, r], r.astype(np.int64)


def near_tie(best, runner):
    """queries whose arg-min fp32 cannot be held to: the float64 gap between best and runner-up is within 2^-18 of the runner-up
    (64 x the fp32 error of the distance expression) -- but not an EXACT tie (duplicate candidates), where the first minimum is
    defined in every arithmetic"""
    with np.errstate(invalid="ignore"):
        gap = runner - best
    return np.isfinite(runner) & (gap > 0) & (gap <= 2.0 ** -18 * runner)


def grad64(P, G, idx1, idx2, scale):
    """per-row gradient of one cloud on GIVEN lists: scale * [ (P_i - G_idx1[i]) + sum_{idx2[j] == i} (P_i - G_j) ] ->
    (gradient (N,3), sum of |terms| (N,3), in-degree (N,))"""
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    own = P - G[idx1]
    acc, mag = own.copy(), np.abs(own)
    deg = np.zeros(len(P), np.int64)
    for j, i in enumerate(np.asarray(idx2)):
        acc[i] += P[i] - G[j]
        mag[i] += np.abs(P[i] - G[j])
        deg[i] += 1
    return scale * acc, mag, deg


def term64(PC, R, t, sym, recon, w, G=None):
    """the term and d term / d recon in float64 (first minima) from the formulas alone, the rows of recon whose gradient hangs on
    a near tie (``near_tie``; (B,N) bool), the sum of |terms| and the in-degree per row.  ``G``: the target to use instead of
    the float64 one (a float32 target promoted: the searches then see the inputs the code under test saw)"""
    if G is None:
        G, _ = target64(PC, R, t, sym)
    G = np.asarray(G, np.float64)
    skip = classes(sym)[3]
    B, N, _ = G.shape
    P = np.asarray(recon, np.float64)
    total, grad, loose = 0.0, np.zeros_like(P), np.zeros((B, N), bool)
    mag, deg = np.zeros_like(P), np.zeros((B, N), np.int64)
    for b in range(B):
        if skip[b]:
            continue
        d1, i1, r1, _ = search64(P[b], G[b])
        d2, i2, r2, k2 = search64(G[b], P[b])
        total += d1.sum() + d2.sum()
        grad[b], mag[b], deg[b] = grad64(P[b], G[b], i1, i2, 2.0 * w / (B * N))
        loose[b] |= near_tie(d1, r1)
        t2 = near_tie(d2, r2)
        loose[b, i2[t2]] = True
        loose[b, k2[t2]] = True
    return w * total / (B * N), grad, loose, mag, deg


def bwd64(x1, x2, idx1, idx2, gd1, gd2):
    """hsp_chamfer_bwd's contract in float64 on given lists, one cloud: (gx1, gx2, sum of |terms| per row of each, in-degrees)"""
    x1, x2, gd1, gd2 = (np.asarray(a, np.float64) for a in (x1, x2, gd1, gd2))
    v1 = 2 * gd1[:, None] * (x1 - x2[idx1])
    v2 = 2 * gd2[:, None] * (x2 - x1[idx2])
    gx1, gx2, m1, m2 = v1.copy(), v2.copy(), np.abs(v1), np.abs(v2)
    c1, c2 = np.zeros(len(x1), np.int64), np.zeros(len(x2), np.int64)
    for i, j in enumerate(np.asarray(idx1)):
        gx2[j] -= v1[i]; m2[j] += np.abs(v1[i]); c2[j] += 1
    for j, i in enumerate(np.asarray(idx2)):
        gx1[i] -= v2[j]; m1[i] += np.abs(v2[j]); c1[i] += 1
    return gx1, gx2, m1, m2, c1, c2


# ---- the batches ---------------------------------------------------------------------------------------------------------------
def batch(ref, B, N, syms, seed=3, tiled=None):
    """clouds of spread 0.05 about z = 0.8 (ref.hash_tensor), a rotation per cloud, recon = target + 0.01 * noise (float32 of the
    float64 target); ``tiled``: that cloud is its first (N + 2) // 3 points repeated, so G and recon hold exact duplicates"""
    PC = ref.hash_tensor((B, N, 3), seed, 0.05) + torch.tensor([0.0, 0.0, 0.8])
    q, _ = torch.linalg.qr(torch.eye(3) + ref.hash_tensor((B, 3, 3), seed + 1, 0.4))
    R = (q * torch.sign(torch.linalg.det(q)).view(B, 1, 1)).contiguous()
    t = (ref.hash_tensor((B, 3), seed + 2, 0.02) + torch.tensor([0.0, 0.0, 0.8])).contiguous()
    sym = torch.tensor([syms[b % len(syms)] for b in range(B)], dtype=torch.float32)
    noise = ref.hash_tensor((B, N, 3), seed + 3, 0.01)
    if tiled is not None:
        base = (N + 2) // 3
        rows = torch.arange(N) % base
        PC[tiled] = PC[tiled, rows]
        noise[tiled] = noise[tiled, rows]
    PC = PC.contiguous()
    G64, _ = target64(PC.numpy(), R.numpy(), t.numpy(), sym.numpy())
    recon = (torch.from_numpy(G64).float() + noise).contiguous()
    return dict(PC=PC, gt_R=R, gt_t=t, sym=sym, recon=recon)


ALL_CLASSES = (SYM_Y, SYM_YX, SYM_NONE, SYM_SKIP)
