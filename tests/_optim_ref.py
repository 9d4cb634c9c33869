"""Shared by the optimizer tests: one Ranger step for one row table stated in numpy float64 WITH a first-order forward error
bound carried next to every value (``step_ref64``), the same formula in numpy float32 in the reference's own operation order
(``step_f32``) with a table of one-line mutants of it (``MUTANTS``), the case table of tests/test_gpu_optim_reference.py
(``cases``), the host scalars of a step as ranger2020.py:194-213 derives them (``radam_scalars``), and the addition count and
the sentinel layout of the gradient-norm kernel (``sumsq_depth``, ``sumsq_input``).  Numpy only: nothing here touches a device.

The formula is tools/torch_utils/solver/ranger2020.py:135-246 and torch.nn.utils.clip_grad_norm_ as restated in
oracle/ref_cpu.py::ranger_step_ / clip_grads_ -- not csrc/optim.hip:

    clip  = min(1, max_norm / (sqrt(gnorm_sq) + 1e-6))                 (only when a squared norm is handed over)
    g     = grad * clip
    g    -= mean(g over the row)                                       (gc rows, gc_loc=True)
    v'    = v * beta2 + (1 - beta2) * g * g
    m'    = m * beta1 + (1 - beta1) * g
    G     = m' / (sqrt(v') + eps)   on an adaptive step,   m'  otherwise (an ALIAS of exp_avg in the reference:
                                                                          what follows then lands in the stored moment)
    G    += weight_decay * p                                           (weight_decay != 0)
    G    -= mean(G over the row)                                       (gc rows, gc_loc=False)
    p'    = p - step_lr * G
    slow' = slow + alpha * (p' - slow);  p' = slow'                    (Lookahead steps)

The bound.  U = 2^-24.  Every input -- the five fp32 arrays, the fp32 scalars the C ABI passes by value, the fp32 squared
norm, the constant 1e-6f -- carries e = 0, and every operation adds its own rounding to what its operands carry:

    a +- b    e = ea + eb + U |a +- b|
    a * b     e = |a| eb + |b| ea + U |a b|
    a / b     e = ea / |b| + |a| eb / b^2 + U |a / b|
    sqrt(a)   e = ea / (2 sqrt a) + U sqrt a          (a = 0:  sqrt(ea))
    row sum   e = sum e_i + D U sum |x_i|,   D = ceil(n / 64) + 6       (a lane's strided partial sum, then the 6-step butterfly)
    min(c, 1) e = ec while c - 2 ec < 1, else 0                         (an fp32 c on the other side of 1 is within ec of 1)

``1 - beta`` is one of these subtractions on the fp32 beta the kernel is handed, so the reference is a function of the ABI's own
arguments.  (ranger2020.py forms 1 - beta2 in double from the double beta2: 1 - fp32(0.999) differs from that by 1.3e-5 relative.
That is a property of passing the betas as floats, it is the same in every step, and it is not what these tests are about.)

A kernel value passes when |kernel - ref64| <= 2 e + 2^-149: the factor 2 stands for the second-order terms a first-order
bound drops, 2^-149 is the smallest fp32 denormal, and no other constant enters.
"""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
F = np.float32
NAMES = ("p", "m", "v", "slow")

Scalars = namedtuple("Scalars", "beta1 beta2 eps weight_decay step_lr adaptive lookahead la_alpha gc_after max_norm")


def scalars(beta1=0.95, beta2=0.999, eps=1e-5, weight_decay=0.0, step_lr=1e-4, adaptive=1, lookahead=0, la_alpha=0.5,
            gc_after=0, max_norm=0.0):
    """the scalar arguments of hsp_ranger_step, the floats already rounded to the fp32 the ABI passes"""
    f = lambda x: float(F(x))
    return Scalars(f(beta1), f(beta2), f(eps), f(weight_decay), f(step_lr), int(adaptive), int(lookahead), f(la_alpha),
                   int(gc_after), f(max_norm))


# ------------------------------------------------------------------------------------------------------------
# float64 values that carry their bound
# ------------------------------------------------------------------------------------------------------------

class V:
    """a float64 value (array or scalar) and the first-order bound on what an fp32 evaluation of it may be off by"""
    __slots__ = ("x", "e")

    def __init__(self, x, e=None):
        self.x = np.asarray(x, dtype=np.float64)
        self.e = np.zeros_like(self.x) if e is None else np.asarray(e, dtype=np.float64)

    def __add__(self, o):
        x = self.x + o.x
        return V(x, self.e + o.e + U * np.abs(x))

    def __sub__(self, o):
        x = self.x - o.x
        return V(x, self.e + o.e + U * np.abs(x))

    def __mul__(self, o):
        x = self.x * o.x
        return V(x, np.abs(self.x) * o.e + np.abs(o.x) * self.e + U * np.abs(x))

    def __truediv__(self, o):
        x = self.x / o.x
        return V(x, self.e / np.abs(o.x) + np.abs(self.x) * o.e / (o.x * o.x) + U * np.abs(x))

    def sqrt(self):
        x = np.sqrt(self.x)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(self.x > 0, self.e / (2 * x) + U * x, np.sqrt(self.e))
        return V(x, e)

    def rowsum(self):
        """sum of a row held by one wave: D = ceil(n / 64) + 6 additions on the longest path"""
        n = self.x.size
        D = (n + 63) // 64 + 6
        return V(self.x.sum(), self.e.sum() + D * U * np.abs(self.x).sum())


def clip_coefficient(gnorm_sq, max_norm):
    """min(1, max_norm / (sqrt(gnorm_sq) + 1e-6f)) with the bounds of its three operations"""
    c = V(max_norm) / (V(float(F(gnorm_sq))).sqrt() + V(float(F(1e-6))))
    if c.x < 1.0:
        return c
    return V(1.0, c.e if c.x - 2 * c.e < 1.0 else 0.0)


def step_ref64(p, g, m, v, slow, rows, sc, gnorm_sq=None):
    """{name: V} over the whole flat buffers for name in p, m, v, slow.  Elements outside every row keep their input value with
    e = 0 (the kernel must leave them alone).  Non-finite inputs propagate as numpy propagates them."""
    out = {k: V(np.asarray(a, np.float64).copy()) for k, a in zip(NAMES, (p, m, v, slow))}
    one = V(1.0)
    b1, b2 = V(sc.beta1), V(sc.beta2)
    omb1, omb2 = one - b1, one - b2
    clip = clip_coefficient(gnorm_sq, sc.max_norm) if gnorm_sq is not None else None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for off, n, gc in rows:
            s = slice(off, off + n)
            w, gr = V(p[s]), V(g[s])
            if clip is not None:
                gr = gr * clip
            if gc and not sc.gc_after:
                gr = gr - gr.rowsum() / V(float(n))
            vn = V(v[s]) * b2 + omb2 * (gr * gr)
            mn = V(m[s]) * b1 + omb1 * gr
            G = mn / (vn.sqrt() + V(sc.eps)) if sc.adaptive else mn
            if sc.weight_decay != 0.0:
                G = G + V(sc.weight_decay) * w
            if gc and sc.gc_after:
                G = G - G.rowsum() / V(float(n))
            w = w - V(sc.step_lr) * G
            if sc.lookahead:
                sl = V(slow[s])
                sl = sl + V(sc.la_alpha) * (w - sl)
                w = sl
                out["slow"].x[s], out["slow"].e[s] = sl.x, sl.e
            stored = mn if sc.adaptive else G
            for k, q in (("p", w), ("m", stored), ("v", vn)):
                out[k].x[s], out[k].e[s] = q.x, q.e
    return out


# ------------------------------------------------------------------------------------------------------------
# the fp32 restatement and its mutants
# ------------------------------------------------------------------------------------------------------------

MUTANTS = {
    "eps_inside_sqrt": "G = m' / sqrt(v' + eps)",
    "mean_over_len_rounded_to_64": "the centralisation mean divides by the row length rounded up to 64",
    "mean_of_unclipped_gradient": "the centralisation mean is taken of grad, not grad * clip",
    "v_from_unclipped_gradient": "exp_avg_sq is updated from the unclipped gradient",
    "row_tail_untouched": "the last len % 64 elements of a row are left as they were",
    "lookahead_one_minus_alpha": "slow' = slow + (1 - alpha) (p' - slow)",
    "nonadaptive_wd_moment_is_mn": "non-adaptive step with weight decay: the stored moment is m', not G",
    "wd_on_updated_weight": "the weight-decay term uses the already-updated weight",
}


def step_f32(p, g, m, v, slow, rows, sc, gnorm_sq=None, mutant=None):
    """{name: float32 array}: the formula of the module docstring in float32, in the reference's operation order, every
    operation rounded once (numpy float32 arithmetic; the row sums are numpy's pairwise float32 sums).  ``mutant``: a key of
    MUTANTS; each is one line that departs from the formula."""
    assert mutant is None or mutant in MUTANTS, mutant
    out = {k: np.array(a, dtype=F, copy=True) for k, a in zip(NAMES, (p, m, v, slow))}
    b1, b2, eps, wd, lr, al = (F(x) for x in (sc.beta1, sc.beta2, sc.eps, sc.weight_decay, sc.step_lr, sc.la_alpha))
    omb1, omb2 = F(1) - b1, F(1) - b2
    clip = None
    if gnorm_sq is not None:
        clip = min(F(sc.max_norm) / (np.sqrt(F(gnorm_sq)) + F(1e-6)), F(1))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for off, n, gc in rows:
            if mutant == "row_tail_untouched": n -= n % 64
            if n == 0:
                continue
            s = slice(off, off + n)
            w, g0 = out["p"][s].copy(), np.asarray(g[s], dtype=F)
            gr = g0 * clip if clip is not None else g0
            gv = gr
            if gc and not sc.gc_after:
                mean = gr.sum(dtype=F) / F(n)
                if mutant == "mean_over_len_rounded_to_64": mean = gr.sum(dtype=F) / F((n + 63) // 64 * 64)
                if mutant == "mean_of_unclipped_gradient": mean = g0.sum(dtype=F) / F(n)
                gr = gr - mean
                gv = gr
                if mutant == "v_from_unclipped_gradient": gv = g0 - mean
            elif mutant == "v_from_unclipped_gradient": gv = g0
            vn = out["v"][s] * b2 + omb2 * (gv * gv)
            mn = out["m"][s] * b1 + omb1 * gr
            G = mn / (np.sqrt(vn) + eps) if sc.adaptive else mn
            if mutant == "eps_inside_sqrt" and sc.adaptive: G = mn / np.sqrt(vn + eps)
            if wd != 0:
                wdw = w
                if mutant == "wd_on_updated_weight": wdw = w - lr * G
                G = G + wd * wdw
            stored = mn if sc.adaptive else G
            if mutant == "nonadaptive_wd_moment_is_mn": stored = mn
            if gc and sc.gc_after:
                G = G - G.sum(dtype=F) / F(n)
                if not sc.adaptive and mutant != "nonadaptive_wd_moment_is_mn":
                    stored = G
            w = w - lr * G
            if sc.lookahead:
                sl = out["slow"][s]
                a = F(1) - al if mutant == "lookahead_one_minus_alpha" else al
                sl = sl + a * (w - sl)
                out["slow"][s] = sl
                w = sl
            out["p"][s], out["m"][s], out["v"][s] = w, stored, vn
    return out


# ------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------

def ratios(got, want):
    """{name: worst |got - ref64| / (2 e + 2^-149)} over every element; a non-finite value on either side counts as
    infinitely far unless both sides are non-finite in the same way"""
    res = {}
    for k in NAMES:
        a, w = np.asarray(got[k], np.float64), want[k]
        with np.errstate(invalid="ignore"):
            r = np.abs(a - w.x) / (2 * w.e + TINY)
        bad = ~np.isfinite(r)
        same = bad & ((np.isnan(a) & np.isnan(w.x)) | (a == w.x))
        r = np.where(same, 0.0, np.where(bad, np.inf, r))
        res[k] = float(r.max()) if r.size else 0.0
    return res


def failures(got, want, limit=5):
    """the elements out of bound, as text (at most ``limit`` per quantity)"""
    msgs = []
    for k in NAMES:
        a, w = np.asarray(got[k], np.float64), want[k]
        with np.errstate(invalid="ignore"):
            err = np.abs(a - w.x)
            bad = ~(err <= 2 * w.e + TINY)
        bad &= ~((np.isnan(a) & np.isnan(w.x)) | (a == w.x))
        idx = np.flatnonzero(bad)
        for i in idx[:limit]:
            msgs.append(f"{k}[{i}]: got {a[i]!r} want {w.x[i]!r} err {err[i]:.3e} bound {2 * w.e[i] + TINY:.3e}")
        if idx.size > limit:
            msgs.append(f"{k}: {idx.size} elements out of bound")
    return msgs


# ------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------

SENTINEL = dict(p=-1234.5, g=777.25, m=3.0e5, v=-9.75e3, slow=4321.125)     # the padding gaps hold these, per buffer

Case = namedtuple("Case", "name rows total p g m v slow sc gnorm_sq gaps")

ROW_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129)
LONG_LENGTHS = (4095, 4096, 4097)
# (len, gc): nine rows of mixed length and kind, a full block of four, a second one, and one row in a third
MIXED = ((70, 1), (5, 0), (64, 1), (1, 1), (200, 1), (65, 0), (3, 1), (129, 1), (257, 0))
TABLES = {
    "short": tuple((n, gc) for n in ROW_LENGTHS for gc in (1, 0)),
    "long_gc": tuple((n, 1) for n in LONG_LENGTHS),
    "long_plain": tuple((n, 0) for n in LONG_LENGTHS),
    "row5000": ((5000, 1),),                        # a row of a 2-D tensor is never cut
    "mixed": MIXED,
}
for _n in (1, 3, 4, 5, 9):                          # around the four-rows-per-block edge
    TABLES[f"rows{_n}"] = MIXED[:_n]


def layout(spec):
    """rows [(offset, len, gc)] and the buffer length for a table spec [(len, gc)]: every start a multiple of 4, a gap of 4 or 8
    elements (plus the fill to the next multiple of 4) before the first row, between rows and after the last"""
    rows, off = [], 4
    for i, (n, gc) in enumerate(spec):
        rows.append((off, n, gc))
        off = ((off + n + 3) & ~3) + 4 * (1 + i % 2)
    return rows, off


# p, g: magnitudes; lr: step_lr; clip: None (no pointer), a float k (max_norm = k * norm: k >= 1 caps at 1) or ("abs", max_norm)
MAGNITUDES = {
    "work":   dict(p=0.1, g=1e-3, warm=True, lr=1e-4, clip=0.5),       # the training point
    "update": dict(p=1.0, g=1.0, warm=True, lr=1.0, clip=None),        # the update is as large as the weight
    "eps":    dict(p=0.1, g=1e-8, warm=True, lr=1e-3, clip=2.0),       # sqrt(v) << eps
    "cold":   dict(p=0.1, g=1e-3, warm=False, lr=1e-4, clip=1e-3),     # m = v = 0, slow = p
    "large":  dict(p=0.1, g=1e4, warm=True, lr=1e-4, clip=("abs", 5.0)),
}
CLIPS = {"noclip": None, "cap": 2.0, "small": 1e-3}


def _signed(rng, n, scale):
    return ((0.25 + 0.75 * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0) * scale).astype(F)


def make_case(name, table, mag, sc_kw, clip="mag", seed=0):
    """the buffers of one case.  The moments of a warm case sit at the scale the CLIPPED gradient drives them to."""
    mg = MAGNITUDES[mag]
    rows, total = layout(TABLES[table])
    rng = np.random.default_rng(1000 + seed)
    clip = mg["clip"] if clip == "mag" else clip
    g = _signed(rng, total, mg["g"])
    inrow = np.zeros(total, bool)
    for off, n, _ in rows:
        inrow[off:off + n] = True
    gnorm_sq, max_norm, coef = None, 0.0, 1.0
    if clip is not None:
        gnorm_sq = F(np.sum(g[inrow].astype(np.float64) ** 2))
        norm = math.sqrt(float(gnorm_sq))
        max_norm = clip[1] if isinstance(clip, tuple) else clip * norm
        coef = min(1.0, max_norm / norm)
    p = _signed(rng, total, mg["p"])
    if mg["warm"]:
        m = _signed(rng, total, 0.3 * mg["g"] * coef)
        v = ((0.5 + rng.random(total)) * (mg["g"] * coef) ** 2).astype(F)
        slow = (p + _signed(rng, total, 0.05 * mg["p"])).astype(F)
    else:
        m, v, slow = np.zeros(total, F), np.zeros(total, F), p.copy()
    bufs = dict(p=p, g=g, m=m, v=v, slow=slow)
    for k, a in bufs.items():
        a[~inrow] = F(SENTINEL[k])
    sc = scalars(step_lr=mg["lr"], max_norm=max_norm, **sc_kw)
    return Case(name, rows, total, p, g, m, v, slow, sc, gnorm_sq, ~inrow)


DEFAULT_MODE = dict()                                                        # adaptive, gc first, no decay, no Lookahead
SECOND_MODE = dict(gc_after=1, weight_decay=0.01, lookahead=1, la_alpha=0.8)

_CASES = None


def cases():
    """the case table, built once: {name: Case}.
      cross/...    the mixed table under adaptive x lookahead x gc_after x weight_decay x clip, at the working point and where
                   the update dominates (Lookahead's alpha is 0.5 at the first and 0.8 at the second)
      len/...      the row-length tables (each length as a gc row and as a plain row, the 5000-element row of a 2-D tensor) in
                   the default mode and in gc_after=1, weight_decay=0.01, lookahead=1, at all five magnitudes
      count/...    1, 3, 4, 5 and 9 rows, both modes, working point and update-dominant"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out, seed = {}, 0
    for mag in ("work", "update"):
        for ad in (0, 1):
            for la in (0, 1):
                for ga in (0, 1):
                    for wd in (0.0, 0.01):
                        for cn, ck in CLIPS.items():
                            seed += 1
                            name = f"cross/{mag}/ad{ad}-la{la}-gcafter{ga}-wd{wd:g}-{cn}"
                            kw = dict(adaptive=ad, lookahead=la, gc_after=ga, weight_decay=wd, la_alpha=0.5 if mag == "work" else 0.8)
                            out[name] = make_case(name, "mixed", mag, kw, clip=ck, seed=seed)
    for table in ("short", "long_gc", "long_plain", "row5000"):
        for mag in MAGNITUDES:
            for mn, kw in (("default", DEFAULT_MODE), ("second", SECOND_MODE)):
                seed += 1
                name = f"len/{table}/{mag}/{mn}"
                out[name] = make_case(name, table, mag, kw, seed=seed)
    for n in (1, 3, 4, 5, 9):
        for mag in ("work", "update"):
            for mn, kw in (("default", DEFAULT_MODE), ("second", SECOND_MODE)):
                seed += 1
                name = f"count/rows{n}/{mag}/{mn}"
                out[name] = make_case(name, f"rows{n}", mag, kw, seed=seed)
    _CASES = out
    return out


_REF = {}


def reference(name):
    """step_ref64 of a case, computed once per process and shared; callers leave it unchanged"""
    if name not in _REF:
        c = cases()[name]
        _REF[name] = step_ref64(c.p, c.g, c.m, c.v, c.slow, c.rows, c.sc, c.gnorm_sq)
    return _REF[name]


# ------------------------------------------------------------------------------------------------------------
# what the Ranger class supplies: the host scalars of a step (ranger2020.py:192-213, 238)
# ------------------------------------------------------------------------------------------------------------

def radam_scalars(step, beta1, beta2, n_sma_threshold=5):
    """(adaptive, step_size) of the 1-based ``step``, in Python doubles as the reference computes them"""
    beta2_t = beta2 ** step
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if N_sma > n_sma_threshold:
        step_size = math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max
                              / (N_sma_max - 2)) / (1 - beta1 ** step)
        return 1, step_size
    return 0, 1.0 / (1 - beta1 ** step)


def class_scalars(step, lr, betas=(0.95, 0.999), eps=1e-5, weight_decay=0.0, alpha=0.5, k=6, n_sma_threshold=5, gc_loc=True,
                  max_norm=0.0):
    """the Scalars of step ``step`` of a Ranger(lr, alpha, k, N_sma_threshhold, betas, eps, weight_decay, gc_loc)"""
    adaptive, step_size = radam_scalars(step, betas[0], betas[1], n_sma_threshold)
    return scalars(beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay, step_lr=step_size * lr, adaptive=adaptive,
                   lookahead=int(step % k == 0), la_alpha=alpha, gc_after=int(not gc_loc), max_norm=max_norm)


ROW_CHUNK = 4096


def expected_rows(shapes, use_gc=True, gc_conv_only=False):
    """[(offset, len, gc)] a flat group of tensors of these shapes must be driven by: tensors start at multiples of 4, a tensor
    of more than one dim gives one row per dim-0 slice, a 1-D tensor is cut at 4096; gc where dim > 1 (conv-only: dim > 3)"""
    rows, off = [], 0
    for sh in shapes:
        n = int(np.prod(sh))
        gc = int(use_gc and len(sh) > (3 if gc_conv_only else 1))
        if len(sh) > 1:
            rl = n // sh[0]
            rows += [(off + r * rl, rl, gc) for r in range(sh[0])]
        else:
            rows += [(off + c, min(ROW_CHUNK, n - c), gc) for c in range(0, n, ROW_CHUNK)]
        off += (n + 3) & ~3
    return rows, off


def row_table_problems(rows, shapes):
    """what is wrong with a row table for tensors of these shapes laid out at 4-element-aligned starts: every parameter element in
    exactly one row, no row on a padding element"""
    total = sum((int(np.prod(s)) + 3) & ~3 for s in shapes)
    owner = np.zeros(total, np.int64)
    msgs = []
    for off, n, _ in rows:
        if off < 0 or n <= 0 or off + n > total:
            msgs.append(f"row ({off}, {n}) outside the buffer of {total}")
            continue
        owner[off:off + n] += 1
    is_param = np.zeros(total, bool)
    o = 0
    for s in shapes:
        n = int(np.prod(s))
        is_param[o:o + n] = True
        o += (n + 3) & ~3
    if (owner[is_param] != 1).any():
        msgs.append(f"{int((owner[is_param] != 1).sum())} parameter elements not in exactly one row")
    if (owner[~is_param] != 0).any():
        msgs.append(f"{int((owner[~is_param] != 0).sum())} padding elements inside a row")
    return msgs, ~is_param


# ------------------------------------------------------------------------------------------------------------
# the gradient norm: hsp_sumsq_f32
# ------------------------------------------------------------------------------------------------------------

SUMSQ_Q = 4 * 256 * 1024                     # the first n that fills the 1024-block grid once
SUMSQ_SIZES = (1, 2, 3, 4, 1023, 1024, 1025, SUMSQ_Q - 4, SUMSQ_Q, SUMSQ_Q + 1, SUMSQ_Q + 4, 3 * SUMSQ_Q + 4 * 256 * 5 + 3)


def sumsq_blocks(n):
    return min(1024, max(1, (n // 4 + 255) // 256))


def sumsq_depth(n):
    """D of |sumsq - sum x^2| <= D U sum x^2, counted from csrc/optim.hip: the longest chain of roundings one x^2 goes through
      1                      the product x * x
      ceil(n4 / (256 nb))    a thread's trips through the float4 loop, one addition per accumulator and trip
      1                      the tail pass of block 0 (at most 3 elements, at most one per thread, into accumulator 0)
      2                      (a0 + a1) + (a2 + a3)
      6                      the wave butterfly
      2                      (red0 + red1) + (red2 + red3)
      ceil(nb / 256)         the second kernel's strided pass over the block partials
      6 + 2                  its butterfly and block fold"""
    nb, n4 = sumsq_blocks(n), n // 4
    trips = (n4 + 256 * nb - 1) // (256 * nb)
    return 1 + trips + 1 + 2 + 6 + 2 + (nb + 255) // 256 + 6 + 2


def sumsq_input(n, seed=0):
    """fp32 data of about 2^-12 with 2^6 where an indexing slip would land, and the sentinel positions"""
    rng = np.random.default_rng(7000 + seed)
    x = ((0.5 + 0.5 * rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0) * 2.0 ** -12).astype(F)
    nb, n4 = sumsq_blocks(n), n // 4
    pos = {0, n - 1}                                  # first, last
    if n4 * 4 < n:
        pos.add(n4 * 4)                               # first tail element
    if n4 > 0:
        pos.add(n4 * 4 - 1)                           # last float4-covered element (the last before the tail)
    pos |= {4 * 256, 4 * 512 - 1}                     # first and last element of block 1's first trip
    pos.add(4 * 256 * nb)                             # first element of the second trip
    pos = sorted(i for i in pos if 0 <= i < n)
    sign = 1.0
    for i in pos:
        x[i] = F(sign * 64.0)
        sign = -sign
    return x, pos
