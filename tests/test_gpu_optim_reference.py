"""GPU: the fused Ranger step (hsp_ranger_step), the gradient norm (hsp_sumsq_f32) and the Ranger class that drives them,
each held to the float64 reference of tests/_optim_ref.py with the bound that module derives: every element of every output
must satisfy |kernel - ref64| <= 2 e + 2^-149.  csrc/optim.hip is built without fused multiply-adds and HIP's fp32 divide and
square root are correctly rounded, so the kernel is a plain fp32 evaluation that differs from the formula only in the order
of its sums: the bound is derived, not tuned (tests/test_optim_reference_host.py shows what it admits and what it rejects).

  1. one step through the C ABI on hand-built row tables: the case table of _optim_ref.cases() (row lengths around the wave
     width and the 1-D chunk size, row counts around the four-rows-per-block edge, the full cross of the modes, five
     magnitudes), padding gaps that hold a sentinel in all five buffers and must come back bit-identical, and the cases whose
     result is exact;
  2. the gradient norm against sum x^2 in float64 up to the grid-stride regime of the real parameter buffer, with 2^6 where an
     indexing slip would land, and the calls it declines;
  3. the Ranger class for 20 steps, re-anchored at every step on the fp32 state read back from the device so that errors never
     compound: step count, rectification switch, Lookahead period, row table, gc flags, per-group learning rate, clip
     hand-over, a schedule, a checkpoint reload, and a non-finite norm;
  4. the worst err / bound ratios measured on the device, printed by the last test (DESIGN.md carries them)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

RATIOS = {}          # quantity -> worst measured |kernel - ref64| / (2 e + 2^-149), printed by the last test
BUFS = ("p", "g", "m", "v", "slow")


def _note(r):
    for k, x in r.items():
        RATIOS[k] = max(RATIOS.get(k, 0.0), x)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _kernel_step(dev, bufs, rows, sc, gnorm_sq=None):
    """hsp_ranger_step on copies of the five host buffers; every buffer as it comes back"""
    from hs_pose_amd import ops
    from hs_pose_amd._lib import HspRowDesc
    total = bufs["p"].size
    assert all(0 <= off and n > 0 and off + n <= total for off, n, _ in rows)          # no row leaves the buffers
    t = {k: torch.from_numpy(np.array(bufs[k], dtype=np.float32, copy=True)).to(dev) for k in BUFS}
    table = ops.upload_table((HspRowDesc * len(rows))(*[(int(o), int(n), int(gc)) for o, n, gc in rows]), dev)
    gn = None if gnorm_sq is None else torch.tensor([float(gnorm_sq)], dtype=torch.float32, device=dev)
    ops._run("hsp_ranger_step",
             (ops._p(t["p"]), ops._p(t["g"]), ops._p(t["m"]), ops._p(t["v"]), ops._p(t["slow"]), ops._p(table), len(rows),
              sc.beta1, sc.beta2, sc.eps, sc.weight_decay, sc.step_lr, sc.adaptive, sc.lookahead, sc.la_alpha, sc.gc_after,
              ops._p(gn), sc.max_norm, ops._stream()))
    return {k: t[k].cpu().numpy() for k in BUFS}


def _run_cases(dev, prefix):
    names = [n for n in R.cases() if n.startswith(prefix)]
    assert names
    bad = []
    for name in names:
        c = R.cases()[name]
        got = _kernel_step(dev, {k: getattr(c, k) for k in BUFS}, c.rows, c.sc, c.gnorm_sq)
        want = R.reference(name)
        bad += [f"{name}: {m}" for m in R.failures(got, want)]
        _note(R.ratios(got, want))
        for k in BUFS:                                           # the gaps, and the whole gradient buffer, bit for bit
            if not (_bits(got[k])[c.gaps] == _bits(np.float32(R.SENTINEL[k]))).all():
                bad.append(f"{name}: a padding element of {k} was written")
        if not np.array_equal(_bits(got["g"]), _bits(c.g)):
            bad.append(f"{name}: the gradient buffer was written")
    assert not bad, "\n".join(bad[:40])
    return len(names)


# ------------------------------------------------------------------------------------------------------------
# 1. one step of the kernel through the C ABI
# ------------------------------------------------------------------------------------------------------------

def test_mode_cross_on_the_mixed_table(dev):
    """adaptive x lookahead x gc_after x weight_decay x clip (no pointer, capped at 1, about 1e-3), at the working point and
    where the update is as large as the weight"""
    assert _run_cases(dev, "cross/") == 96


@pytest.mark.parametrize("table", ["short", "long_gc", "long_plain", "row5000"])
def test_row_lengths(dev, table):
    """1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097 as gc rows and as plain rows, a gc row of 5000; the default mode and
    gc_after=1, weight_decay=0.01, lookahead=1; working point, update-dominant, eps-dominant, cold start, large gradients"""
    assert _run_cases(dev, f"len/{table}/") == 10


def test_row_counts(dev):
    """1, 3, 4, 5 and 9 rows: the last block of four waves is partly idle"""
    assert _run_cases(dev, "count/") == 20


def _small(seed, spec, lookahead=0, adaptive=1, zero_moments=False, zero_grad=False, slow_is_p=False, **kw):
    rows, total = R.layout(spec)
    rng = np.random.default_rng(seed)
    b = dict(p=R._signed(rng, total, 0.1), g=R._signed(rng, total, 1e-2), m=R._signed(rng, total, 3e-3),
             v=(rng.random(total) * 1e-4 + 1e-5).astype(np.float32), slow=R._signed(rng, total, 0.1))
    if zero_moments:
        b["m"][:] = 0; b["v"][:] = 0
    if zero_grad:
        b["g"][:] = 0
    if slow_is_p:
        b["slow"] = b["p"].copy()
    return b, rows, R.scalars(step_lr=1e-2, lookahead=lookahead, adaptive=adaptive, **kw)


@pytest.mark.parametrize("clip", [None, 0.37])
def test_exact_gc_row_of_one_element(dev, clip):
    """the centralised gradient of a one-element row is g - g / 1 = 0 exactly: m' = beta1 m and v' = beta2 v bit for bit
    (one rounding each), and from m = 0 the weight does not move"""
    spec = ((1, 1), (1, 1), (1, 1), (1, 1), (1, 1))
    for zero_moments in (False, True):
        b, rows, sc = _small(11, spec, zero_moments=zero_moments, max_norm=1.0 if clip else 0.0)
        got = _kernel_step(dev, b, rows, sc, None if clip is None else np.float32((1.0 / clip) ** 2))
        idx = [off for off, _, _ in rows]
        assert np.array_equal(_bits(got["m"][idx]), _bits(b["m"][idx] * np.float32(sc.beta1)))
        assert np.array_equal(_bits(got["v"][idx]), _bits(b["v"][idx] * np.float32(sc.beta2)))
        if zero_moments:
            assert np.array_equal(_bits(got["p"]), _bits(b["p"]))
        assert not R.failures(got, R.step_ref64(b["p"], b["g"], b["m"], b["v"], b["slow"], rows, sc,
                                                None if clip is None else np.float32((1.0 / clip) ** 2)))


@pytest.mark.parametrize("lookahead", [0, 1])
def test_exact_zero_gradient_from_zero_moments(dev, lookahead):
    """g = 0, m = v = 0: G = 0 / (0 + eps) = 0, p is unchanged; slow is untouched without Lookahead and, holding p, unchanged
    with it"""
    b, rows, sc = _small(12, R.MIXED, lookahead=lookahead, zero_moments=True, zero_grad=True, slow_is_p=bool(lookahead))
    got = _kernel_step(dev, b, rows, sc)
    for k in BUFS:
        assert np.array_equal(_bits(got[k]), _bits(b[k])), k


@pytest.mark.parametrize("gc_after", [0, 1])
def test_exact_slow_untouched_without_lookahead(dev, gc_after):
    b, rows, sc = _small(13, R.MIXED, lookahead=0, gc_after=gc_after, weight_decay=0.01)
    got = _kernel_step(dev, b, rows, sc)
    assert np.array_equal(_bits(got["slow"]), _bits(b["slow"]))
    assert not np.array_equal(_bits(got["p"]), _bits(b["p"]))


@pytest.mark.parametrize("gc_after", [0, 1])
@pytest.mark.parametrize("adaptive", [0, 1])
def test_exact_lookahead_hands_the_slow_weights_back(dev, adaptive, gc_after):
    """lookahead=1: p' is slow' bit for bit (here with alpha = 1), and both are within the bound of the reference"""
    b, rows, sc = _small(14, R.MIXED, lookahead=1, la_alpha=1.0, adaptive=adaptive, gc_after=gc_after)
    got = _kernel_step(dev, b, rows, sc)
    for off, n, _ in rows:
        assert np.array_equal(_bits(got["p"][off:off + n]), _bits(got["slow"][off:off + n]))
    assert not R.failures(got, R.step_ref64(b["p"], b["g"], b["m"], b["v"], b["slow"], rows, sc))


# ------------------------------------------------------------------------------------------------------------
# 2. the gradient norm
# ------------------------------------------------------------------------------------------------------------

def _sumsq(dev, x):
    from hs_pose_amd import ops
    from hs_pose_amd._lib import lib
    n = x.numel()
    assert x.data_ptr() % 16 == 0
    out = torch.full((1,), -1.0, device=dev)
    wsb = lib().hsp_sumsq_workspace_bytes(n)
    assert wsb == 4 * R.sumsq_blocks(n)
    ws = ops._ws(wsb, dev)
    ops._run("hsp_sumsq_f32", (ops._p(x), n, ops._p(out), ops._p(ws), wsb, ops._stream()))
    return float(out.double().cpu())


@pytest.mark.parametrize("n", R.SUMSQ_SIZES)
def test_sumsq_against_float64(dev, n):
    """|kernel - sum x^2| <= 2 D U sum x^2 + 2^-149 with D counted from the kernel (_optim_ref.sumsq_depth); 2^6 among 2^-12 at
    element 0, the last, the first tail element, the last float4-covered one, both ends of block 1's first trip and the first
    element of the second trip: one of them dropped or counted twice moves the sum by a seventh or more"""
    x, pos = R.sumsq_input(n, seed=n % 97)
    want = float((x.astype(np.float64) ** 2).sum())
    got = _sumsq(dev, torch.from_numpy(x).to(dev))
    bound = 2 * R.sumsq_depth(n) * R.U * want + R.TINY
    r = abs(got - want) / bound
    print(f"\nsumsq n={n}: {len(pos)} sentinels, D={R.sumsq_depth(n)}, err/bound {r:.3f}")
    RATIOS["sumsq"] = max(RATIOS.get("sumsq", 0.0), r)
    assert r <= 1.0, (n, got, want, bound)
    assert 4096.0 > 10 * bound                                   # a sentinel is visible


def test_sumsq_declines(dev):
    """unaligned start -> unsupported, n <= 0 -> bad argument, short workspace -> workspace error; ``out`` is not written"""
    from hs_pose_amd import _lib, ops
    L = _lib.lib()
    buf = torch.ones(4100, device=dev)
    out = torch.full((1,), -7.5, device=dev)
    n = 4096
    wsb = L.hsp_sumsq_workspace_bytes(n)
    ws = ops._ws(wsb, dev)

    def call(x, n_, wsb_):
        return L.hsp_sumsq_f32(ops._p(x), n_, ops._p(out), ops._p(ws), wsb_, ops._stream())
    assert L.hsp_sumsq_workspace_bytes(0) == 0
    for k in (1, 2, 3):
        assert call(buf[k:], n, wsb) == _lib.ERR_UNSUPPORTED
    assert call(buf, 0, wsb) == _lib.ERR_BAD_ARG
    assert call(buf, -1, wsb) == _lib.ERR_BAD_ARG
    assert call(buf, n, wsb - 1) == _lib.ERR_WORKSPACE
    assert call(buf, n, 0) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert float(out) == -7.5
    assert call(buf, n, wsb) == 0 and float(out) == float(n)


# ------------------------------------------------------------------------------------------------------------
# 3. the Ranger class, re-anchored each step
# ------------------------------------------------------------------------------------------------------------

SHAPES = [(4, 6), (5, 3, 1), (7,), (3, 2, 2, 2), (9, 70), (4200,), (2, 130), (1,), (3, 1)]
SHAPES_B = [(6, 65), (5,), (2, 3, 4)]


def _new_params(dev, shapes, seed):
    rng = np.random.default_rng(seed)
    return [torch.nn.Parameter(torch.from_numpy(R._signed(rng, int(np.prod(s)), 0.1).reshape(s)).to(dev)) for s in shapes]


def _flat_state(fg):
    return {k: t.cpu().numpy() for k, t in zip(BUFS, (fg.flat_p, fg.flat_g, fg.flat_m, fg.flat_v, fg.flat_s))}


def _gnorm_check(opt, pre):
    """the squared norm clip_grad_norm_ left on the device against float64 over every group: each group's own reduction, plus
    the one addition per extra group of the stacked sum"""
    got = float(opt._gnorm_sq.double().cpu())
    parts = [float((np.float64(s["g"]) ** 2).sum()) for s in pre]
    e = sum(R.sumsq_depth(s["g"].size) * R.U * x for s, x in zip(pre, parts)) + (len(parts) - 1) * R.U * sum(parts)
    r = abs(got - sum(parts)) / (2 * e + R.TINY)
    RATIOS["sumsq"] = max(RATIOS.get("sumsq", 0.0), r)
    assert r <= 1.0, (got, sum(parts))
    return np.float32(got)


def _drive(dev, groups, opt_kw, *, max_norm=None, lr_lambda=None, reload_at=None, steps=20, seed=0):
    """``steps`` steps of Ranger over ``groups`` = [(shapes, lr)]; before each, the fp32 state is read back and the step
    expected of exactly that state is computed in float64 (scalars from _optim_ref.class_scalars, rows from
    _optim_ref.expected_rows -- neither from solver.py)"""
    from hs_pose_amd.solver import Ranger
    params = [_new_params(dev, shapes, seed + 10 * i) for i, (shapes, _) in enumerate(groups)]
    make = lambda ps: Ranger([dict(params=p, lr=lr) for p, (_, lr) in zip(ps, groups)], **opt_kw)
    opt = make(params)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda) if lr_lambda else None
    use_gc, conv_only = opt_kw.get("use_gc", True), opt_kw.get("gc_conv_only", False)
    ref_kw = dict(eps=opt_kw.get("eps", 1e-5), weight_decay=opt_kw.get("weight_decay", 0.0), alpha=opt_kw.get("alpha", 0.5),
                  k=opt_kw.get("k", 6), gc_loc=opt_kw.get("gc_loc", True))
    tables = [R.expected_rows(shapes, use_gc, conv_only) for shapes, _ in groups]
    pads = [R.row_table_problems(rows, shapes)[1] for (rows, _), (shapes, _) in zip(tables, groups)]
    rng = np.random.default_rng(seed + 1)
    fresh = True                                   # the slow weights are taken from the weights at the first step
    seen = set()
    for step in range(1, steps + 1):
        for fg in opt._flat:
            for p in fg.params:
                p.grad.copy_(torch.from_numpy(R._signed(rng, p.numel(), 1e-2).reshape(p.shape)).to(dev))
        gsq = None
        if max_norm is not None:
            opt.clip_grad_norm_(max_norm)
        pre = [_flat_state(fg) for fg in opt._flat]
        if max_norm is not None:
            gsq = _gnorm_check(opt, pre)
        opt.step()
        for gi, (fg, s, (rows, total), (shapes, lr)) in enumerate(zip(opt._flat, pre, tables, groups)):
            assert fg.total == total
            lr_now = lr * (lr_lambda(step - 1) if lr_lambda else 1.0)
            sc = R.class_scalars(step, lr_now, max_norm=max_norm or 0.0, **ref_kw)
            seen.add((sc.adaptive, sc.lookahead))
            slow = s["p"] if fresh else s["slow"]
            want = R.step_ref64(s["p"], s["g"], s["m"], s["v"], slow, rows, sc, gsq)
            got = _flat_state(fg)
            bad = R.failures(got, want)
            assert not bad, (f"step {step} group {gi}", bad)
            _note(R.ratios(got, want))
            for k in BUFS:
                assert not got[k][pads[gi]].any(), (step, gi, k, "padding element not zero")
            assert all(opt.state[p]["step"] == step for p in fg.params)
        fresh = False
        if sch is not None:
            sch.step()
        if step == reload_at:
            sd = copy.deepcopy(opt.state_dict())
            sd["state"] = {k: {n: (v.cpu().clone() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()}
            old = [_flat_state(fg) for fg in opt._flat]
            params = [[torch.nn.Parameter(p.detach().clone()) for p in fg.params] for fg in opt._flat]
            opt = make(params)
            opt.load_state_dict(sd)
            for fg, o in zip(opt._flat, old):
                new = _flat_state(fg)
                for k in ("p", "m", "v", "slow"):
                    assert np.array_equal(_bits(new[k]), _bits(o[k])), k
    assert seen >= {(0, 0), (1, 0), (1, 1)}, seen
    return opt


CLASS_CONFIGS = {
    "defaults": dict(groups=[(SHAPES, 1e-3)], opt_kw={}, max_norm=0.05),
    "no_gc": dict(groups=[(SHAPES, 1e-3)], opt_kw=dict(use_gc=False), max_norm=0.05),
    "conv_only": dict(groups=[(SHAPES, 1e-3)], opt_kw=dict(gc_conv_only=True)),
    "gc_after_wd": dict(groups=[(SHAPES, 1e-3)], opt_kw=dict(gc_loc=False, weight_decay=0.01), max_norm=1e9),
    "alpha0.8_k3": dict(groups=[(SHAPES, 1e-3)], opt_kw=dict(alpha=0.8, k=3)),
    "two_groups": dict(groups=[(SHAPES, 1e-3), (SHAPES_B, 3e-2)], opt_kw={}, max_norm=0.05),
    "lambda_lr": dict(groups=[(SHAPES, 1e-2)], opt_kw={}, lr_lambda=lambda x: 1.0 / (1.0 + 0.37 * x), max_norm=0.05),
    "reload": dict(groups=[(SHAPES, 1e-3), (SHAPES_B, 1e-2)], opt_kw=dict(k=4), reload_at=10, max_norm=0.05),
}


@pytest.mark.parametrize("name", list(CLASS_CONFIGS))
def test_ranger_class_step_by_step(dev, name):
    c = dict(CLASS_CONFIGS[name])
    _drive(dev, c.pop("groups"), c.pop("opt_kw"), seed=sum(map(ord, name)), **c)


def _resolved(fg, use_gc, conv_only):
    raw = fg.rows_for(use_gc, conv_only).cpu().numpy().tobytes()
    a = np.frombuffer(raw, dtype=np.dtype([("offset", "<i8"), ("len", "<i4"), ("gc", "<i4")]))
    return [(int(o), int(n), int(g)) for o, n, g in a]


def _check_tables(fg):
    from hs_pose_amd._lib import HspRowDesc
    assert ctypes.sizeof(HspRowDesc) == 16
    shapes = [tuple(p.shape) for p in fg.params]
    want, total = R.expected_rows(shapes)
    assert fg.total == total and fg.nrows == len(want)
    assert [tuple(r) for r in fg.rows_host] == want
    assert not R.row_table_problems(fg.rows_host, shapes)[0]
    for p, o in zip(fg.params, fg.offsets):
        if p.dim() == 1:                                         # 1-D tensors are cut at 4096
            mine = [n for off, n, _ in fg.rows_host if o <= off < o + p.numel()]
            assert max(mine) <= R.ROW_CHUNK and sum(mine) == p.numel()
    for use_gc, conv_only in ((True, False), (True, True), (False, False), (False, True)):
        assert _resolved(fg, use_gc, conv_only) == R.expected_rows(shapes, use_gc, conv_only)[0], (use_gc, conv_only)


def test_row_tables(dev, flags):
    """every parameter element in exactly one row, no row on a padding element, gc where dim > 1 (conv-only: dim > 3), 1-D
    tensors cut at 4096: for the tensor sets above and for the real network"""
    from hs_pose_amd.HSPose import HSPose
    from hs_pose_amd.solver import Ranger, build_optimizer
    for shapes in (SHAPES, SHAPES_B, [(4097,), (8193,), (4096,), (3,)]):
        _check_tables(Ranger(_new_params(dev, shapes, 5), lr=1e-3)._flat[0])
    flags.train = 1
    net = HSPose("PoseNet_only").to(dev)
    opt = build_optimizer(net.build_params(training_stage_freeze=[]))
    assert sum(fg.total for fg in opt._flat) > 9e6
    for fg in opt._flat:
        _check_tables(fg)


def _pair(dev, shapes, grads, max_norm, scale_first):
    from hs_pose_amd.solver import Ranger
    params = _new_params(dev, shapes, 21)
    opt = Ranger(params, lr=1e-2)
    for p, g in zip(params, grads):
        p.grad.copy_(g.to(dev))
    opt.clip_grad_norm_(max_norm)
    pre = _flat_state(opt._flat[0])
    gsq = np.float32(float(opt._gnorm_sq.cpu()))
    if scale_first:
        opt.scale_grads_by_clip_()
        assert opt._gnorm_sq is None
    opt.step()
    return pre, gsq, _flat_state(opt._flat[0])


@pytest.mark.parametrize("max_norm", [0.05, 1e9])
def test_clip_hand_over_paths_agree(dev, max_norm):
    """clip_grad_norm_ -> scale_grads_by_clip_ -> step (the iteration only accumulated) and clip_grad_norm_ -> step (the kernel
    applies the coefficient) both land within the bound of the same float64 step"""
    rng = np.random.default_rng(31)
    grads = [torch.from_numpy(R._signed(rng, int(np.prod(s)), 1e-2).reshape(s)) for s in SHAPES]
    rows, _ = R.expected_rows(SHAPES)
    res = []
    for scale_first in (True, False):
        pre, gsq, got = _pair(dev, SHAPES, grads, max_norm, scale_first)
        sc = R.class_scalars(1, 1e-2, max_norm=max_norm)
        want = R.step_ref64(pre["p"], pre["g"], pre["m"], pre["v"], pre["p"], rows, sc, gsq)
        assert not R.failures(got, want), (scale_first, R.failures(got, want))
        _note(R.ratios(got, want))
        res.append(got)
    same = all(np.array_equal(_bits(res[0][k]), _bits(res[1][k])) for k in R.NAMES)
    print(f"\nclip hand-over, max_norm={max_norm}: the two paths are {'bit-equal' if same else 'NOT bit-equal'}")


@pytest.mark.parametrize("poison", ["nan", "inf"])
def test_non_finite_norm_follows_torch(dev, poison):
    """one NaN / one +inf gradient element: the gradients torch.nn.utils.clip_grad_norm_ leaves on CPU copies decide which
    elements of p, m and v may be finite after the step, on both clip paths (a NaN norm poisons every gradient; an infinite
    one zeroes all but the infinite element).  Non-finite numbers go through arithmetic only; no index depends on them."""
    shapes = [(4, 6), (7,), (3, 2, 2, 2), (130,)]
    rng = np.random.default_rng(41)
    grads = [torch.from_numpy(R._signed(rng, int(np.prod(s)), 1e-2).reshape(s)) for s in shapes]
    grads[0][1, 2] = float("nan") if poison == "nan" else float("inf")
    max_norm = 0.05
    cpu = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for p, g in zip(cpu, grads):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(cpu, max_norm)
    rows, total = R.expected_rows(shapes)
    pad = R.row_table_problems(rows, shapes)[1]
    g_want = np.zeros(total, np.float32)
    g_want[~pad] = np.concatenate([p.grad.numpy().ravel() for p in cpu])
    for scale_first in (True, False):
        pre, gsq, got = _pair(dev, shapes, grads, max_norm, scale_first)
        want = R.step_ref64(pre["p"], g_want, pre["m"], pre["v"], pre["p"], rows, R.class_scalars(1, 1e-2))
        if scale_first:
            assert np.array_equal(np.isfinite(got["g"])[~pad], np.isfinite(g_want)[~pad]), "scale_grads_by_clip_ vs torch"
        for k in ("p", "m", "v"):
            a, b = np.isfinite(got[k]), np.isfinite(want[k].x)
            assert np.array_equal(a, b), (f"{k}: {int((a != b).sum())} elements finite on one side only "
                                          f"({'scale_grads_by_clip_' if scale_first else 'in-kernel clip'} path)")
        fin = np.isfinite(want["p"].x)[~pad]
        assert fin.any() == (poison == "inf") and not fin.all()


# ------------------------------------------------------------------------------------------------------------
# 4. record
# ------------------------------------------------------------------------------------------------------------

def test_zz_report_worst_ratios():
    """worst |kernel - ref64| / (2 e + 2^-149) seen by the tests above, per quantity (DESIGN.md carries these figures)"""
    print("\nworst err / bound on the device:")
    for k in ("p", "m", "v", "slow", "sumsq"):
        if k in RATIOS:
            print(f"  {k:6s} {RATIOS[k]:.3f}")
            assert RATIOS[k] <= 1.0
