"""The libhsp calls behind the public ops, as data: for a fixed list of small cases, the ordered (entry point, key, abytes, aflops)
records a forward + backward leaves in an ``ops.KernelTimer`` and, where the results are run-to-run reproducible, the sha256 of every
output and gradient.  tests/test_gpu_call_records.py compares a fresh run with tests/golden/call_records.json, so a change to how
ops.py marshals an entry point that alters a call, its order, its roofline figures or a single bit of a result is seen.

    python tools/record_op_calls.py tests/golden/call_records.json        # (re)write the fixture -- from the commit it speaks for

Inputs come from a seeded CPU generator (one seed per case name: a case does not depend on which others ran) and are uploaded.
Only public names of ``ops`` / ``ops_bf16`` are used.  A case runs under each mode it lists: a module switch or FLAGS field set for
its extent, or (``exact``) inside ``ops.exact_scope`` with autograd recording -- the layer nodes' own exact forward.
Gradients are left out of the hashes where a backward adds in arrival order (the default pooling backward with a per-query
gradient, ``hsp_gather_rows_bwd``): there the records alone are compared.
"""
import contextlib
import hashlib
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, BF = torch.float32, torch.bfloat16
B, K, C = 2, 20, 128          # clouds, neighbours, channels
N_CHUNKED, N_COUNTS = 64, 160  # below / above ops.ORL_COUNTS_MIN_N: the chunked ORL forward, the slab form that leaves counts

# every switch a case may be run under: name -> (owner, attribute, value); owner "scope": the context manager of ``ops`` by that name
MODES = {"default": None, "det": ("ops", "DETERMINISTIC", True), "repro": ("flags", "reproducible", True),
         "nocounts": ("ops", "ORL_COUNTS", False), "rider": ("ops", "COLSUM_RIDER", True),
         "exact": ("scope", "exact_scope", True), "nodiet": ("ops", "LAUNCH_DIET", False)}
GEOMETRY = ("default", "det", "repro")        # pooling / ORL / receptive-field / row-gather cases run under all three
TAILS = ("exact", "nodiet")                   # the layer nodes' exact-scope forward (autograd recording) and four-launch chain
CASES = {}                                    # "<case>/<mode>" -> (function, mode)


def case(*modes):
    def deco(fn):
        for m in modes or ("default",):
            CASES[f"{fn.__name__}/{m}"] = (fn, m)
        return fn
    return deco


class Inputs:
    """seeded CPU draws, uploaded"""

    def __init__(self, dev, name):
        self.dev, self.g = dev, torch.Generator().manual_seed(zlib.crc32(name.encode()))

    def randn(self, *shape, scale=1.0, dtype=F32, grad=False, shift=0.0):
        return (torch.randn(*shape, generator=self.g) * scale + shift).to(self.dev, dtype).requires_grad_(grad)

    def ints(self, hi, *shape):
        return torch.randint(0, hi, shape, generator=self.g, dtype=torch.int32).to(self.dev)

    def kept(self, n, nq, clouds=0):
        """nq distinct rows of n: one list, or one per cloud"""
        rows = [torch.randperm(n, generator=self.g)[:nq] for _ in range(max(clouds, 1))]
        return (torch.stack(rows) if clouds else rows[0]).to(torch.int32).to(self.dev)

    def bn(self, c, train=True):
        m = torch.nn.BatchNorm1d(c)
        with torch.no_grad():
            m.weight.copy_(torch.randn(c, generator=self.g) * 0.2 + 1)
            m.bias.copy_(torch.randn(c, generator=self.g) * 0.2)
            m.running_mean.copy_(torch.randn(c, generator=self.g) * 0.1)
            m.running_var.copy_(torch.rand(c, generator=self.g) + 0.5)
        return m.to(self.dev).train(train)

    def like(self, t):
        return torch.randn(t.shape, generator=self.g).to(t.device, t.dtype)


def _copies(*weights):
    """bf16 working copies (both forms) of 2-D fp32 weights / column blocks, refreshed; the caller keeps the result alive"""
    from hs_pose_amd import ops_bf16
    reg = ops_bf16.Bf16Params([(w.detach(), True, True) for w in weights])
    reg.refresh()
    return reg


# ---- receptive field, layers ---------------------------------------------------------------------------------------------------

def _layer_params(inp, cin, S, surface=False):
    p = dict(directions=inp.randn(3, S * C, grad=True), w_conv2=inp.randn(C, 2 * C, 1, scale=C ** -0.5, grad=True),
             w_ste=inp.randn(C, 3 if surface else cin, 1, scale=0.1, grad=True))
    if not surface:
        p.update(weights=inp.randn(cin, (S + 1) * C, scale=cin ** -0.5, grad=True), bias=inp.randn((S + 1) * C, scale=0.1, grad=True))
    return p


def _S():
    from hs_pose_amd.config import FLAGS
    return FLAGS.gcn_sup_num


@case(*GEOMETRY)
def rf_surface(inp):
    from hs_pose_amd import ops
    xyz, idx, d = inp.randn(B, N_CHUNKED, 3, scale=0.1), inp.ints(N_CHUNKED, B, N_CHUNKED, K), inp.randn(3, _S() * C, grad=True)
    return (lambda: [ops.rf_surface(xyz, idx, d, _S())]), [d]


@case(*GEOMETRY)
def rf_conv(inp):
    from hs_pose_amd import ops
    S = _S()
    xyz, idx, d = inp.randn(B, N_CHUNKED, 3, scale=0.1), inp.ints(N_CHUNKED, B, N_CHUNKED, K), inp.randn(3, S * C, grad=True)
    fm = inp.randn(B, N_CHUNKED, (S + 1) * C, grad=True)
    return (lambda: [ops.rf_conv(xyz, idx, d, fm, S)]), [d, fm]


def _surface(inp, n, dtype, relu):
    from hs_pose_amd import ops
    S = _S()
    xyz, idx, p = inp.randn(B, n, 3, scale=0.1), inp.ints(n, B, n, K), _layer_params(inp, 3, S, surface=True)
    keep = _copies(p["w_conv2"].squeeze(-1)) if dtype == BF else None

    def fwd():
        out = ops.surface_layer(xyz, idx, K, S, p["directions"], p["w_ste"], p["w_conv2"], relu=relu, out_dtype=dtype)
        return list(out) if isinstance(out, tuple) else [out]
    fwd.keep = keep
    return fwd, list(p.values())


@case(*GEOMETRY, *TAILS)
def surface_layer_f32(inp):
    return _surface(inp, N_CHUNKED, F32, False)


@case(*GEOMETRY, "nocounts", *TAILS)
def surface_layer_f32_relu_counts(inp):
    return _surface(inp, N_COUNTS, F32, True)


@case(*GEOMETRY, "nocounts")
def surface_layer_bf16(inp):
    return _surface(inp, N_COUNTS, BF, False)


def _hs(inp, b, n, dtype, bn_shift=False, out_f32=False):
    from hs_pose_amd import ops
    S = _S()
    xyz, idx_f, idx_x = inp.randn(b, n, 3, scale=0.1), inp.ints(n, b, n, K), inp.ints(n, b, n, K)
    X, p = inp.randn(b, n, C, dtype=dtype, grad=True), _layer_params(inp, C, S)
    keep = _copies(p["weights"], p["w_ste"].squeeze(-1), p["w_conv2"].squeeze(-1)) if dtype == BF else None

    def fwd():
        out = ops.hs_layer(xyz, X, idx_f, idx_x, K, S, p["weights"], p["bias"], p["directions"], p["w_ste"], p["w_conv2"],
                           bn_shift=True if bn_shift else None, out_f32=out_f32)
        return list(out) if isinstance(out, tuple) else [out]
    fwd.keep = keep
    return fwd, [X] + list(p.values())


@case(*GEOMETRY, *TAILS)
def hs_layer_f32_chunked(inp):
    return _hs(inp, B, N_CHUNKED, F32)


@case(*GEOMETRY, "nocounts", *TAILS)
def hs_layer_f32_counts(inp):
    return _hs(inp, B, N_COUNTS, F32)


@case("default", "nocounts")
def hs_layer_f32_bn_shift(inp):
    return _hs(inp, B, N_COUNTS, F32, bn_shift=True)


@case(*GEOMETRY, "nocounts")
def hs_layer_bf16(inp):
    return _hs(inp, B, N_COUNTS, BF)


@case("default")
def hs_layer_f32_bn_shift_x3(inp):
    """8192 rows of 128 columns: the fewest from which the out product runs on the x3 kernel that leaves the BatchNorm partials"""
    return _hs(inp, 16, 512, F32, bn_shift=True)


@case("default")
def hs_layer_bf16_out_f32(inp):
    return _hs(inp, B, N_COUNTS, BF, out_f32=True)


@case("default", "rider", "det")
def hs_layer_f32_16_clouds(inp):
    """16 clouds: the per-cloud chain of the backward in two launches, and (``rider``) its column sum inside the pair launch"""
    return _hs(inp, 16, N_CHUNKED, F32)


# ---- pooling, ORL, row gathers -------------------------------------------------------------------------------------------------

def _gather_max(inp, dtype, sel):
    from hs_pose_amd import ops
    n, nq = N_CHUNKED, 24
    feat, idx = inp.randn(B, n, C, dtype=dtype, grad=True), inp.ints(n, B, n, K)
    qsel = None if sel is None else inp.kept(n, nq, B if sel == "cloud" else 0)
    return (lambda: [ops.gather_max(feat, idx, 4, qsel)]), [feat]


for _dt, _dn in ((F32, "f32"), (BF, "bf16")):
    for _sel in (None, "shared", "cloud"):
        def _f(inp, _dt=_dt, _sel=_sel):
            return _gather_max(inp, _dt, _sel)
        _f.__name__ = f"gather_max_{_dn}_{_sel or 'all'}"
        case(*GEOMETRY)(_f)


def _pool(inp, clouds):
    from hs_pose_amd import ops
    n = N_CHUNKED
    feat, xyz, idx = inp.randn(B, n, C, grad=True), inp.randn(B, n, 3, scale=0.1), inp.ints(n, B, n, K)
    qsel = inp.kept(n, 16, clouds)
    return (lambda: list(ops.pool_layer(feat, xyz, idx, qsel, 4))), [feat]


@case(*GEOMETRY)
def pool_layer_shared(inp):
    return _pool(inp, 0)


@case(*GEOMETRY)
def pool_layer_per_cloud(inp):
    return _pool(inp, B)


@case(*GEOMETRY, "nocounts")
def orl_global(inp):
    from hs_pose_amd import ops
    feat, idx = inp.randn(B, N_COUNTS, C, grad=True), inp.ints(N_COUNTS, B, N_COUNTS, K)
    return (lambda: [ops.orl_global(feat, idx, K)]), [feat]


@case(*GEOMETRY)
def gather_rows_per_cloud(inp):
    from hs_pose_amd import ops
    feat, idx = inp.randn(B, N_CHUNKED, C, grad=True), inp.ints(N_CHUNKED, B, N_COUNTS)
    return (lambda: [ops.gather_rows(feat, idx)]), [feat]


@case(*GEOMETRY)
def gather_rows_shared(inp):
    from hs_pose_amd import ops
    feat, idx = inp.randn(B, N_CHUNKED, C, grad=True), inp.ints(N_CHUNKED, N_COUNTS)
    return (lambda: [ops.gather_rows(feat, idx)]), [feat]


def _assemble(inp, dtype, gathered):
    """cat[direct, gathered rows ..., one-hot id]; ``gathered``: widths of the gathered segments"""
    from hs_pose_amd import ops
    n = N_COUNTS
    direct = inp.randn(B, n, 64, dtype=dtype, grad=True)
    srcs = [inp.randn(B, N_CHUNKED, w, dtype=dtype, grad=True) for w in gathered]
    up = inp.ints(N_CHUNKED, B, n)
    ids = torch.tensor([1.0, 4.0], device=inp.dev)
    segs = [(direct, None, 0)] + [(s, up, 1) for s in srcs] + [(ids, None, 3)]
    return (lambda: [ops.assemble_feat(segs)]), [direct] + srcs


@case(*GEOMETRY)
def assemble_feat_one_gathered(inp):
    return _assemble(inp, F32, (128,))


@case(*GEOMETRY)
def assemble_feat_two_gathered(inp):
    return _assemble(inp, F32, (128, 256))


@case(*GEOMETRY)
def assemble_feat_narrow_gathered(inp):
    return _assemble(inp, F32, (3,))


@case("default")
def assemble_feat_bf16(inp):
    return _assemble(inp, BF, (128,))


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------

def _bn(inp, dtype, train=True, **kw):
    from hs_pose_amd import ops
    x, bn = inp.randn(B, N_COUNTS, C, dtype=dtype, grad=train, shift=2.0), inp.bn(C, train)

    def fwd():
        out = ops.bn_relu(x, bn, **kw)
        return (list(out) if isinstance(out, tuple) else [out]) + [bn.running_mean, bn.running_var]
    return fwd, [x, bn.weight, bn.bias]


@case()
def bn_relu_train_f32(inp):
    return _bn(inp, F32)


@case()
def bn_relu_train_bf16(inp):
    return _bn(inp, BF)


@case()
def bn_relu_train_mixed(inp):
    return _bn(inp, F32, out_dtype=BF)


@case()
def bn_relu_train_fork(inp):
    return _bn(inp, F32, fork=True)


@case()
def bn_relu_eval_bf16(inp):
    return _bn(inp, BF, train=False)


@case()
def bn_relu_eval_mixed(inp):
    return _bn(inp, F32, train=False, out_dtype=BF)


@case()
def linear_bn_partials(inp):
    """a K = 512 -> N = 512 Linear whose product leaves the BatchNorm's first pass, and the BatchNorm that folds it"""
    from hs_pose_amd import ops
    x, w, b, bn = inp.randn(2048, 512, grad=True), inp.randn(512, 512, scale=512 ** -0.5, grad=True), inp.randn(512, grad=True), inp.bn(512)

    def fwd():
        y, part = ops.linear_rows(x, w, b, bn_partials=True)
        return [ops.bn_relu(y, bn, partial=part), part]
    return fwd, [x, w, b, bn.weight, bn.bias]


# ---- the bf16 heads ------------------------------------------------------------------------------------------------------------

def _grad_mode(train, f):
    """``f`` as it is (train) or under no_grad (eval: these nodes have no backward through running statistics)"""
    def fwd():
        with torch.set_grad_enabled(train):
            return f()
    return fwd


def _dense_bn(inp, train):
    from hs_pose_amd import ops_bf16
    x, w, b, bn = inp.randn(B * N_COUNTS, C, dtype=BF, grad=train), inp.randn(256, C, scale=C ** -0.5, grad=True), \
        inp.randn(256, grad=True), inp.bn(256, train)
    keep = _copies(w)
    fwd = _grad_mode(train, lambda: [ops_bf16.dense_bn(x, w, b, bn)])
    fwd.keep = keep
    return fwd, ([x, w, b, bn.weight, bn.bias] if train else [])


@case()
def dense_bn_train(inp):
    return _dense_bn(inp, True)


@case()
def dense_bn_eval(inp):
    return _dense_bn(inp, False)


def _cloud_cat_bn(inp, train):
    from hs_pose_amd import ops_bf16
    n, cg, cx, cout = N_COUNTS, 128, 128, 128
    fg, x, xyz = inp.randn(B, cg, grad=train), inp.randn(B * n, cx, dtype=BF, grad=train), inp.randn(B, n, 3, scale=0.1)
    W, b, bn = inp.randn(cout, cg + cx + 3, scale=0.1, grad=True), inp.randn(cout, grad=True), inp.bn(cout, train)
    keep = _copies(W[:, cg:cg + cx])
    fwd = _grad_mode(train, lambda: [ops_bf16.cloud_cat_bn(fg, x, xyz, W, b, bn)])
    fwd.keep = keep
    return fwd, ([fg, x, W, b, bn.weight, bn.bias] if train else [])


@case()
def cloud_cat_bn_train(inp):
    return _cloud_cat_bn(inp, True)


@case()
def cloud_cat_bn_eval(inp):
    return _cloud_cat_bn(inp, False)


def _fan_bn(inp, train):
    from hs_pose_amd import ops_bf16
    n, k = N_COUNTS, 128
    x, xyz = inp.randn(B * n, k, dtype=BF, grad=train), inp.randn(B, n, 3, scale=0.1)
    layers = [(inp.randn(128, k + (3 if i == 1 else 0), scale=0.1, grad=True), inp.randn(128, grad=True), inp.bn(128, train))
              for i in range(3)]
    keep = _copies(*[w[:, :k] for w, _, _ in layers])
    fwd = _grad_mode(train, lambda: list(ops_bf16.fan_bn(x, xyz, layers)))
    fwd.keep = keep
    return fwd, ([x] + [t for w, b, bn in layers for t in (w, b, bn.weight, bn.bias)] if train else [])


@case()
def fan_bn_train(inp):
    return _fan_bn(inp, True)


@case()
def fan_bn_eval(inp):
    return _fan_bn(inp, False)


# ---- dense products ------------------------------------------------------------------------------------------------------------

@case()
def linear_rows(inp):
    from hs_pose_amd import ops
    x, w, b = inp.randn(B * N_COUNTS, C, grad=True), inp.randn(256, C, scale=C ** -0.5, grad=True), inp.randn(256, grad=True)
    return (lambda: [ops.linear_rows(x, w, b)]), [x, w, b]


@case()
def gemm_rows_f32(inp):
    from hs_pose_amd import ops
    m = 130
    a1, a2 = inp.randn(m, 96), inp.randn(m, 40)
    w_nt, w_nn, w2 = inp.randn(C, 96), inp.randn(96, C), inp.randn(C, 40)
    bias, resid = inp.randn(C), inp.randn(m, C)
    return (lambda: [ops.gemm_rows(a1, w_nt), ops.gemm_rows(a1, w_nn, nn1=True, alpha=0.5),
                     ops.gemm_rows(a1, w_nt, False, a2, w2, False, bias=bias, resid=resid)]), []


@case()
def gemm_rows_bf16(inp):
    from hs_pose_amd import ops
    m = 136
    a1, a2, w1, w2 = inp.randn(m, 96, dtype=BF), inp.randn(m, 64, dtype=BF), inp.randn(C, 96, dtype=BF), inp.randn(C, 64, dtype=BF)
    bias = inp.randn(C)
    return (lambda: [ops.gemm_rows(a1, w1, bias=bias), ops.gemm_rows(a1, w1, False, a2, w2, False, out=torch.empty(m, C, device=inp.dev))]), []


@case()
def gemm_wave(inp):
    """one source (K, N), two sources (K, N) + (N, K), one source (N, K) with a bias: three of the kernel's forms"""
    from hs_pose_amd import ops
    m = 192
    a1, a2, w_nn, w_nt, w2, bias = inp.randn(m, 96), inp.randn(m, 64), inp.randn(96, C), inp.randn(C, 96), inp.randn(C, 64), inp.randn(C)
    return (lambda: [ops.gemm_wave(a1, w_nn, True), ops.gemm_wave(a1, w_nn, True, a2, w2, False),
                     ops.gemm_wave(a1, w_nt, False, bias=bias)]), []


@case()
def gemm_x3(inp):
    """(2048, 512): 128 tiles of 64 x 128, the fewest the x3 kernels take with an epilogue"""
    from hs_pose_amd import ops
    m, n = 2048, 512
    a1, a2, w1, w2 = inp.randn(m, 96), inp.randn(m, 64), inp.randn(96, n), inp.randn(n, 64)
    bias, resid, cb = inp.randn(n), inp.randn(m, n), inp.randn(2, n)

    def fwd():
        outs = [ops.gemm_x3(a1, w1, True, bias=bias),
                ops.gemm_x3(a1, w1, True, a2, w2, False, resid=resid, cloud_bias=cb, rows_per_cloud=m // 2)]
        ops.x3_refresh()                       # the registry's one re-split launch over both matrices
        return outs + [ops.gemm_x3(a1, w1, True)]
    return fwd, []


@case()
def gemm_rows_acc(inp):
    from hs_pose_amd import ops_bf16
    m = 136
    a1, a2, w1, w2 = inp.randn(m, 96, dtype=BF), inp.randn(m, 64, dtype=BF), inp.randn(C, 96, dtype=BF), inp.randn(C, 64, dtype=BF)
    resid = inp.randn(m, C)
    return (lambda: [ops_bf16.gemm_rows_acc(a1, w1, a2, w2, resid, torch.empty(m, C, device=inp.dev)),
                     ops_bf16.gemm_rows_acc(a1, w1, None, None, resid, torch.empty(m, C, dtype=BF, device=inp.dev))]), []


# ---- the recorder --------------------------------------------------------------------------------------------------------------

def _sha(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def adds_in_arrival_order(calls):
    """True where a call list holds a backward whose fp32 sums depend on the order the waves arrive in"""
    for name, key, _, _ in calls:
        if name == "hsp_gather_rows_bwd":
            return True
        if name.startswith("hsp_gather_max_bwd") and "csr" not in name and not key.endswith(("bc", "bc+", "cnt+")):
            return True
    return False


@contextlib.contextmanager
def _mode(switch):
    """the case's switch set for the extent of the block"""
    from hs_pose_amd import ops
    from hs_pose_amd.config import FLAGS
    if switch is None:
        yield
    elif switch[0] == "scope":
        with getattr(ops, switch[1])(switch[2]):
            yield
    else:
        owner = ops if switch[0] == "ops" else FLAGS
        before = getattr(owner, switch[1])
        setattr(owner, switch[1], switch[2])
        try:
            yield
        finally:
            setattr(owner, switch[1], before)


def run_case(name, dev):
    """{"calls": [[entry point, key, abytes, aflops], ...], "outputs": [sha256, ...], "grads": [sha256 | None, ...] | None}"""
    from hs_pose_amd import ops
    fn, mode = CASES[name]
    timer = ops.KernelTimer()
    with _mode(MODES[mode]):
        with ops.x3_scope(ops.X3Planes()):          # a registry of its own: the split launches do not depend on earlier cases
            inp = Inputs(dev, name.split("/")[0])
            fwd, leaves = fn(inp)
            prev = ops.set_timer(timer)
            try:
                outs = fwd()
                diff = [o for o in outs if o.requires_grad]
                if diff:
                    torch.autograd.backward(diff, [inp.like(o) for o in diff])
            finally:
                ops.set_timer(prev)
            torch.cuda.synchronize()
    calls = [[n, k, int(ab), int(fl)] for n, k, ab, fl, _, _ in timer.records]
    grads = None
    if leaves and not adds_in_arrival_order(calls):
        grads = [None if t.grad is None else _sha(t.grad) for t in leaves]
    return dict(calls=calls, outputs=[_sha(o) for o in outs], grads=grads)


def record(dev, names=None):
    return {name: run_case(name, dev) for name in (names or sorted(CASES))}


def entry_points(records):
    """every entry-point name that occurs in a set of records"""
    return sorted({c[0] for r in records.values() for c in r["calls"]})


def main(argv):
    from hs_pose_amd._lib import HspError
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "call_records.json")
    got, failed = {}, []
    for name in sorted(CASES):
        try:
            got[name] = run_case(name, torch.device("cuda:0"))
        except HspError as e:                       # a declined call (nothing ran): list every such case, write no fixture
            failed.append(f"{name}: {e}")
            if "[hip:" in str(e):                   # a launch that failed is no decline: stop here
                break
    if failed:
        sys.exit("\n".join(failed))
    with open(out, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases, {sum(len(r['calls']) for r in got.values())} calls, {len(entry_points(got))} entry points -> {out}")


if __name__ == "__main__":
    main(sys.argv)
