"""References of the row-copy, column-sum and reverse-index kernels (csrc/gather.hip outside its scatter-tile / ORL / points-max
part, csrc/csr.hip), written from the formulas of include/hsp.h in numpy / torch on the CPU.  Nothing here imports the package
or calls a kernel: the plan of a column sum (rows per chunk, chunks, row lanes) is an ARGUMENT, which the tests fetch from
hsp_colsum_rows_plan.  tests/test_rows_reference_host.py holds these functions to independent torch compositions;
tests/test_gpu_rows_reference.py holds the kernels to them.

    column sums     want[b,c] = sum_i x[b,i,c] in fp64 of the stored values (bf16 widened exactly); moment slot q = 1..3:
                    sum_i x[b,i,c] * xyz[b,i,q-1], the product in fp64.  Bound per element D u T / (1 - D u), u = 2^-24,
                    T = sum_i |t_i|, D = ceil(rows / row_lanes) + (row_lanes - 1) + ceil(nchunk / 8) + 3 (the additions on the
                    longest path of the documented order), D + 1 for a moment slot (the product's rounding).
    row assembly    a plain indexed copy (kind 0 / 1 / 2 / 3 of hsp_concat_rows)
    row gather      out[b,q] = feat[b, idx[b,q]]; backward = fp64 index_add (atomic form) or a serial fp32 sum in ascending
                    query order (the gather form over the reverse map)
    reverse map     off = [0, cumsum(bincount(targets))], edge = stable argsort of the targets
    fused passes    out + (f + t[b]) in fp32;  (ga + gb) * [y > 0] in fp32
"""
import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64
BF = torch.bfloat16


# ---- column sums ------------------------------------------------------------------------------------------------------------------

def colsum_depth(rows, row_lanes, nchunk):
    """D: the additions on the longest path of the documented order"""
    return -(-rows // row_lanes) + (row_lanes - 1) + -(-nchunk // 8) + 3


def colsum_terms(x, xyz=None):
    """the fp64 terms t (B,N,C) or, with xyz, (B,N,4,C): slot 0 the stored value, slot q the fp64 product with coordinate q-1"""
    t = x.to(F64)
    if xyz is None:
        return t
    w = xyz.to(F64)
    return torch.stack([t] + [t * w[:, :, q:q + 1] for q in range(3)], 2)


def colsum_ref(x, xyz=None):
    """(want, T): fp64 sums over the rows and the sums of the terms' magnitudes; (B,C) or (B,4,C)"""
    t = colsum_terms(x, xyz)
    return t.sum(1), t.abs().sum(1)


def colsum_tol(T, D, moments=False):
    """per-element bound; moments: T (B,4,C), slots 1..3 get D + 1"""
    def one(d):
        return d * U / (1 - d * U)
    if not moments:
        return one(D) * T
    f = torch.tensor([one(D)] + [one(D + 1)] * 3, dtype=F64).view(1, 4, 1)
    return f * T


def edge_rows(N, rows, nchunk):
    """rows of a cloud a chunked sum can lose or double at an edge: every chunk's last row, the cloud's last row, the last
    chunk's first row"""
    e = {N - 1, (nchunk - 1) * rows}
    e.update(min(N, (c + 1) * rows) - 1 for c in range(nchunk))
    return sorted(r for r in e if 0 <= r < N)


def colsum_data(B, N, C, kind, seed, rows, nchunk, dtype=torch.float32, with_xyz=False, quiet=0):
    """(x (B,N,C) as stored, xyz (B,N,3) or None).  kind "range": column c scaled by 2^((7c mod 41) - 20); "cancel": rows in
    +- pairs plus a residue 2^-12 of the scale.  Ordinary rows stay within 4 scales (times 2^-quiet: the clouds of thousands of
    chunks, whose bound would otherwise pass a quarter of any single term); every EDGE row of every column carries
    +-8 .. 16 scales, so a column's largest term sits on an edge row and losing or doubling any one edge row moves the sum by
    that much.  xyz: ordinary rows inside (-1, 1), edge rows of magnitude 1 .. 2 per coordinate (the same for the moments)."""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 ** ((7 * torch.arange(C) % 41) - 20).double()
    z = torch.randn(B, N, C, generator=g, dtype=F64).clamp_(-4, 4) * 2.0 ** -quiet
    if kind == "cancel":
        h = N // 2
        z[:, h:2 * h] = -z[:, :h] + 2.0 ** -12 * torch.randn(B, h, C, generator=g, dtype=F64)
        z.clamp_(-4, 4)
        z = z[:, torch.randperm(N, generator=g)]
    else:
        assert kind == "range"
    er = torch.tensor(edge_rows(N, rows, nchunk))
    sign = torch.where(torch.rand(B, len(er), C, generator=g) < 0.5, -1.0, 1.0).double()
    z[:, er] = sign * (8 + 8 * torch.rand(B, len(er), C, generator=g, dtype=F64))
    x = (z * scale).to(torch.float32).to(dtype)
    xyz = None
    if with_xyz:
        xyz = 2 * torch.rand(B, N, 3, generator=g) - 1
        s3 = torch.where(torch.rand(B, len(er), 3, generator=g) < 0.5, -1.0, 1.0)
        xyz[:, er] = s3 * (1 + torch.rand(B, len(er), 3, generator=g))
    return x, xyz


def colsum_condition(x, xyz, N, rows, nchunk, D):
    """what keeps the bound meaningful, None when it holds, else a message: in every column (and slot) the bound is at most a
    quarter of the column's largest |t_i|, and that largest term sits on an edge row"""
    t = colsum_terms(x, xyz).abs()                                       # (B,N,C) or (B,N,4,C)
    mom = xyz is not None
    tol = colsum_tol(t.sum(1), D, mom)
    big, where = t.max(1)
    if not bool((tol <= big / 4).all()):
        return f"bound above a quarter of the largest term: worst ratio {(tol / big).max().item():.3g}"
    er = torch.zeros(N, dtype=torch.bool)
    er[edge_rows(N, rows, nchunk)] = True
    if not bool(er[where].all()):
        return "a column's largest term is not on an edge row"
    return None


# ---- row assembly -----------------------------------------------------------------------------------------------------------------

def concat_form(elem_bytes, pitch, segs, out_addr):
    """the form hsp_concat_rows* documents for a call: "v16" (16-byte chunks), "pair" (two elements) or "scalar".
    segs: [(kind, width, source address)], pitch in elements.  Pair: even pitch, an output base on two elements, and every
    kind 0 / 1 segment of even width at an even column on a two-element base.  v16: the pair conditions and the same with 16
    bytes -- pitch, the output base and every kind 0 / 1 segment's width, column and base multiples of 16 bytes."""
    def ok(unit_bytes):
        e = unit_bytes // elem_bytes
        if pitch % e or out_addr % unit_bytes:
            return False
        col = 0
        for kind, width, addr in segs:
            if kind < 2 and (width % e or col % e or addr % unit_bytes):
                return False
            col += width
        return True
    if not ok(2 * elem_bytes):
        return "scalar"
    return "v16" if ok(16) else "pair"


def concat_ref(segs, B, N):
    """segs: [dict(kind, width, src, idx, nsrc)] with src a torch tensor -- kind 0: (B*N, w), kind 1: (B*nsrc, w) and idx (B*N)
    rows of the cloud, kind 2: (B, w) fp32, kind 3: (B,) fp32 category ids -- -> (B*N, sum w) of the dtype of the kind 0 / 1
    sources (fp32 when there are none); a kind 2 / 3 fp32 value is converted to that dtype"""
    dt = next((s["src"].dtype for s in segs if s["kind"] < 2), torch.float32)
    cloud = torch.arange(B * N) // N
    cols = []
    for s in segs:
        k, w, src = s["kind"], s["width"], s["src"]
        if k == 0:
            cols.append(src.reshape(B * N, w))
        elif k == 1:
            cols.append(src.reshape(-1, w)[cloud * s["nsrc"] + s["idx"].reshape(-1).long()])
        elif k == 2:
            cols.append(src.reshape(B, w)[cloud].to(dt))
        else:
            ids = src.reshape(B).double().trunc()[cloud]                 # (long) id: truncation toward zero
            cols.append((ids[:, None] == torch.arange(w).double()[None, :]).to(dt))
    return torch.cat(cols, 1)


# ---- row gather -------------------------------------------------------------------------------------------------------------------

def _per_cloud(idx, B):
    idx = torch.as_tensor(idx).long()
    return idx.expand(B, -1) if idx.dim() == 1 else idx


def gather_fwd_ref(feat, idx):
    """feat (B,Nsrc,C), idx (B,Nq) or shared (Nq) -> (B,Nq,C), a copy"""
    B = feat.shape[0]
    ix = _per_cloud(idx, B)
    return torch.stack([feat[b][ix[b]] for b in range(B)])


def gather_bwd_ref(g, idx, Nsrc):
    """g (B,Nq,C) -> (want (B,Nsrc,C) fp64, T = sum|g| of each cell, n (B,Nsrc) list lengths)"""
    B, Nq, C = g.shape
    ix = _per_cloud(idx, B)
    want = torch.zeros(B, Nsrc, C, dtype=F64)
    T = torch.zeros(B, Nsrc, C, dtype=F64)
    n = torch.zeros(B, Nsrc, dtype=F64)
    for b in range(B):
        want[b].index_add_(0, ix[b], g[b].to(F64))
        T[b].index_add_(0, ix[b], g[b].to(F64).abs())
        n[b].index_add_(0, ix[b], torch.ones(Nq, dtype=F64))
    return want, T, n


def gather_bwd_serial(g, rev_off, rev_edge, Nsrc):
    """the gather form: g (B,Nq,C) fp32 or bf16 as stored; every cell one fp32 sum from +0 over the row's list in list order
    (ascending query), stored as is (fp32) or rounded once to nearest even (bf16) -> (B,Nsrc,C) of g's dtype"""
    B, Nq, C = g.shape
    gv = g.float().numpy()
    off, edge = np.asarray(rev_off), np.asarray(rev_edge)
    out = np.zeros((B, Nsrc, C), np.float32)
    for b in range(B):
        ln = off[b, 1:] - off[b, :-1]
        for p in range(int(ln.max()) if Nsrc else 0):
            m = np.nonzero(ln > p)[0]
            out[b, m] = (out[b, m] + gv[b, edge[b, off[b, m] + p]]).astype(np.float32)
    return torch.from_numpy(out).to(g.dtype)


# ---- reverse map ------------------------------------------------------------------------------------------------------------------

def rev_ref(targets, Nsrc):
    """targets (B,E): the source row of edge e -> (rev_off (B,Nsrc+1), rev_edge (B,E)) int32"""
    targets = np.asarray(targets)
    B, E = targets.shape
    off = np.zeros((B, Nsrc + 1), np.int32)
    edge = np.empty((B, E), np.int32)
    for b in range(B):
        off[b, 1:] = np.cumsum(np.bincount(targets[b], minlength=Nsrc))
        edge[b] = np.argsort(targets[b], kind="stable")
    return off, edge


def rev_targets(idx, k, qsel=None):
    """idx (B,Nidx,kstride) -> (B, Nq*k): the source row of edge e = q*k + n; qsel None, (Nq,) shared or (B,Nq) per cloud"""
    idx = np.asarray(idx)
    B = idx.shape[0]
    if qsel is None:
        return idx[:, :, :k].reshape(B, -1)
    qs = np.asarray(qsel)
    qs = np.broadcast_to(qs, (B, qs.shape[-1])) if qs.ndim == 1 else qs
    return np.stack([idx[b, qs[b], :k].reshape(-1) for b in range(B)])


# ---- the two fused passes ---------------------------------------------------------------------------------------------------------

def residual_bias_ref(out, f, t):
    """fp32: out + (f + t[b]), both additions rounded"""
    o, ff, tt = (np.asarray(a, dtype=np.float32) for a in (out, f, t))
    inner = (ff + tt[:, None, :]).astype(np.float32)
    return (o + inner).astype(np.float32)


def add_relu_bwd_ref(ga, gb, y):
    """fp32: (ga + gb) where y > 0 (a positive subnormal counts; +-0 and NaN do not), else +0"""
    a = np.asarray(ga, dtype=np.float32)
    if gb is not None:
        a = (a + np.asarray(gb, dtype=np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(y, dtype=np.float32) > 0, a, np.float32(0)).astype(np.float32)


# ---- the column-sum cases, shared by the host test (the condition) and the GPU test (the kernels) ------------------------------------

FORMS = ("rows", "rows_bf16", "xyz", "xyz_bf16")
VEC_WIDTHS = (4, 8, 64, 128, 512, 1024)
SCALAR_WIDTHS = (1, 3, 6, 48, 100, 255)
CHUNKS = (1, 7, 8, 9, 32, 33)                  # 33: "one above 32"; (2, 5000, 64) is a case of its own


def pick_n(plan, B, C, elem_bytes, nchunk, exact):
    """the smallest N whose plan has `nchunk` chunks with N == rows * nchunk (exact) or N == rows * (nchunk - 1) + 1, found by
    asking `plan(B, N, C, elem_bytes) -> (rows, nchunk, row_lanes, form)`; None when no N up to 8192 has it"""
    for N in range(1, 8193):
        rows, nc, _, _ = plan(B, N, C, elem_bytes)
        if nc == nchunk and N == (rows * nchunk if exact else rows * (nchunk - 1) + 1):
            return N
    return None


def colsum_cases(plan, form, C):
    """[(B, N, data kind, seed)] of one (form, width): every chunk count of CHUNKS at both N (picked from the plan), N = 1, 2, the
    shape (3, 7) below the row lanes, B = 1 and 3 and both data sets in turn; the widest rows keep B = 1 past 32 chunks"""
    eb = 2 if form.endswith("bf16") else 4
    out, i = [], 0
    for nchunk in CHUNKS:
        for exact in (True, False):
            B = 1 if (i % 2 == 0 or (nchunk > 32 and C >= 512)) else 3
            N = pick_n(plan, B, C, eb, nchunk, exact)
            if N is not None and (B, N) not in [(b, n) for b, n, _, _ in out]:
                out.append((B, N, ("range", "cancel")[(i // 2 + i) % 2], 1000 * C + i))
            i += 1
    out += [(3, 1, "range", 1000 * C + 90), (1, 2, "cancel", 1000 * C + 91), (3, 7, "range", 1000 * C + 92)]
    if C == 64:
        out.append((2, 5000, "cancel", 1000 * C + 93))
    return out


CLOUD_WIDTHS = (32, 64, 128, 1024)


def cloud_limits(ok):
    """(largest N accepted, first N refused) of `ok(N) -> 0 / 1` (hsp_colsum_cloud_ok at fixed B, C, with_xyz), found by asking:
    N = 1 .. 8192 one by one (the chunking is not monotone in N there), then doubling and bisection (from 4096 rows on the
    rows per chunk are at their cap and the chunk count only grows).  Probes past the answer must all be refused."""
    small = [N for N in range(1, 8193) if ok(N)]
    refused = next((N for N in range(1, 8193) if not ok(N)), None)
    if len(small) == 8192 or ok(8193):
        lo, hi = 8193 if ok(8193) else 8192, 16384
        while ok(hi):
            lo, hi = hi, 2 * hi
            assert hi < 1 << 26
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        largest = lo
        refused = hi if refused is None else refused
    else:
        largest = small[-1]
    assert ok(largest) and not ok(largest + 1) and not ok(refused) and all(ok(N) for N in range(1, refused))
    assert not any(ok(N) for N in (largest + 2, largest + 127, largest + 128, largest + 129, 2 * largest, 4 * largest + 1, 1 << 20))
    return largest, refused


def cloud_cases(plan, ok, C, with_xyz):
    """[(B, N, data kind, seed, quiet, accepted)] of the one-launch form at width C: the cases of colsum_cases it accepts, then
    the largest N it accepts and the first it refuses at B = 1"""
    out = [(B, N, kind, seed + 7, 0, True) for B, N, kind, seed in colsum_cases(plan, "rows", C) if ok(B, N, C, with_xyz)]
    largest, refused = cloud_limits(lambda N: ok(1, N, C, with_xyz))
    out.append((1, largest, "range", 1000 * C + 95, 10, True))
    out.append((1, refused, "range", 1000 * C + 96, 10, False))
    return out
