"""bf16 feature storage for the HS stack (BASELINE.json configs[3]: dense clouds, "KNN LDS tiling + MFMA MLP path").

What is bf16: the layer inputs / outputs, ``fm = X W + b`` and the winners' support values ``fwin``, every activation
gradient, and the GEMM operands (working copies of the weights, made once per step from the fp32 master parameters by
ONE ``hsp_cast_params_bf16`` launch).  What stays fp32: xyz, the support directions and theta -- the reference hard-casts
the receptive field with ``.float()`` (network/fs_net_repo/gcn3d.py:57,59) --, neighbour indices / arg-max, BatchNorm
statistics and affine parameters, the per-cloud ORL rows (B,C), every parameter gradient and the master parameters
themselves (state_dict unchanged).  Every kernel accumulates in fp32.

The HS layers themselves are the nodes of ``ops`` (``ops.hs_layer`` / ``ops.surface_layer`` take fp32 or bf16 rows: the same chain
on the ``*_bf16`` entry points, the products reading the working copies below).  This module holds those working copies and the
heads, which are different nodes in the two dtypes.
"""
import weakref

import torch

from . import ops
from ._lib import HspCastDesc, HspCastPitchedDesc, HspError, lib
from .ops import _copies, _p, _req, _run, _stream, _ws, copies_of, upload_table

BF16 = torch.bfloat16


class Bf16Params:
    """bf16 working copies (and (N,K)-form transposes) of the GEMM weights of a module tree, refreshed by one launch.

    ``specs``: list of (parameter viewed as a 2-D fp32 matrix, want_copy, want_transposed[, pitched]).  ``pitched``: the copy's
    rows sit on a 16-byte pitch (a K = 1286 weight: the bf16 GEMM's (N,K) operand must be 16-byte aligned); any pitched entry
    makes the one refresh launch ``hsp_cast_params_pitched_bf16``."""

    def __init__(self, specs):
        dev = specs[0][0].device
        me = weakref.ref(self)
        self.entries = []
        self.pitched = any(len(sp) > 3 and sp[3] for sp in specs)
        tab = ((HspCastPitchedDesc if self.pitched else HspCastDesc) * len(specs))()
        tiles = 0
        for i, sp in enumerate(specs):
            w2, want, want_t = sp[:3]
            if w2.dim() != 2 or w2.dtype != torch.float32 or w2.stride(1) != 1:
                raise HspError("Bf16Params: fp32 matrices with contiguous rows")
            rows, cols = w2.shape
            ldd = (cols + 7) // 8 * 8 if len(sp) > 3 and sp[3] else cols
            c = torch.empty(rows, ldd, dtype=BF16, device=dev)[:, :cols] if want else None
            ct = torch.empty(cols, rows, dtype=BF16, device=dev) if want_t else None
            self.entries.append((w2, c, ct))
            _copies[w2.data_ptr()] = (c, ct, me)
            row = (w2.data_ptr(), c.data_ptr() if c is not None else 0, ct.data_ptr() if ct is not None else 0, rows, cols,
                   w2.stride(0), tiles)
            tab[i] = row + ((ldd, rows) if self.pitched else ())          # src, dst, dstT, rows, cols, ld, tile0[, ldd, lddT]
            tiles += ((rows + 31) // 32) * ((cols + 31) // 32)
        self.total_tiles = tiles
        self.n = len(specs)
        self.table = upload_table(tab, dev)
        self.ptrs = [w2.data_ptr() for w2, _, _ in self.entries]
        weakref.finalize(self, Bf16Params._release, self.ptrs, me).atexit = False

    @staticmethod
    def _release(ptrs, me):
        """this Bf16Params is gone (weakref.finalize): its copies leave the registry (an address a later one took over stays)"""
        for ptr in ptrs:
            if ptr in _copies and _copies[ptr][2] is me:
                del _copies[ptr]

    def refresh(self):
        """round the current fp32 master weights into the working copies (call at the top of every forward)"""
        for (w2, _, _), ptr in zip(self.entries, self.ptrs):
            if w2.data_ptr() != ptr:
                raise HspError("Bf16Params: a parameter was re-seated (e.g. by building the fused optimizer); rebuild the "
                               "bf16 copies with FaceRecon.set_feature_dtype(torch.bfloat16)")
        _run("hsp_cast_params_pitched_bf16" if self.pitched else "hsp_cast_params_bf16",
             (_p(self.table), self.n, self.total_tiles, _stream()), key=f"n{self.n}",
             abytes=6 * sum(w.numel() for w, _, _ in self.entries))


def _b(t, name):
    return _req(t, BF16, name)


# ------------------------------------------------------------------------------------------------
# the heads on bf16 rows (PoseR.py / PoseTs.py / FaceRecon.py:37-68): every Conv1d(k=1) + BatchNorm + ReLU as ONE node
#   forward   y = x W^T + b  (+ xyz3 . w3) (+ per-cloud bias)   hsp_gemm_rows_bn_bf16, fp32 out (it feeds BatchNorm) + the
#                                                              BatchNorm's first pass in the epilogue (train mode)
#             a = relu(bn(y))                                  hsp_bn_relu_fwd_partials_mixed (train: fold + apply) /
#                                                              hsp_bn_relu_apply_mixed (eval), bf16
#   backward  g = bn_relu_bwd(da)                              hsp_bn_relu_bwd_mixed, bf16
#             gx = g W                                         hsp_gemm_rows_bf16 on the transposed working copy
#             gW^T, gb = x^T g, colsum(g)                      hsp_wgrad_bf16 / hsp_wgrad_ragged_bf16 (fp32)
# One node per layer: y's gradient never exists in fp32 (a separate BatchNorm node would hand an fp32 y a bf16 gradient that
# autograd widens, and the product would round it back).
# ------------------------------------------------------------------------------------------------

def _bn_fwd(y, bn):
    """relu(bn(y)) for fp32 rows y (R, C) -> (bf16 rows, saved mean, saved invstd); eval mode: running statistics (no saved)"""
    R, C = y.shape
    if not _bn_ok(bn, R, C):
        raise HspError("bf16 heads: this BatchNorm configuration is not built")
    if not bn.training:
        return ops._bn_apply_raw(y, bn.running_mean, _eval_invstd(bn), bn.weight, bn.bias, True), None, None
    return ops._bn_fwd_raw(y, _bn_state(bn), True, BF16)


def _bn_state(bn):
    """a BatchNorm module's tensors and constants as ``ops._bn_fwd_raw`` takes them"""
    return bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum


def _eval_invstd(bn):
    """1 / sqrt(running_var + eps) of an eval-mode BatchNorm, cached on the module until the running variance changes (an
    inference forward reads it without launching anything)"""
    rv = bn.running_var
    key = (rv.data_ptr(), rv._version, float(bn.eps))
    hit = getattr(bn, "_hsp_invstd_bf16", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    inv = torch.rsqrt(rv.detach() + bn.eps)
    bn._hsp_invstd_bf16 = (key, inv)
    return inv


def _bn_ok(bn, R, C):
    return bn.affine and bn.track_running_stats and bn.momentum is not None and ops._bn_takes(R, C)


def _product_bn(x, Wc, b, bn, out_cols, cloud_bias=None, rows_per_cloud=0, xyz3=None, w3=None):
    """y = x Wc^T + b (+ cloud_bias[row // rows_per_cloud]) (+ xyz3 . w3) in fp32 and a = relu(bn(y)) in bf16 -> (a, y, saved mean,
    saved invstd).  Train mode: the product leaves the BatchNorm's first pass in its epilogue (hsp_gemm_rows_bn_bf16) and
    ``ops._bn_fwd_raw`` folds it and applies (y is read once); eval mode / more row tiles than the fold takes:
    hsp_gemm_rows_bf16 + _bn_fwd."""
    R, K = x.shape
    C = out_cols
    y = torch.empty(R, C, dtype=torch.float32, device=x.device)
    L = lib()
    tiles = L.hsp_gemm_rows_bn_tiles_bf16(R, C, K)
    if not (bn.training and _bn_ok(bn, R, C) and tiles > 0):
        ops.gemm_rows(x, Wc, bias=b, cloud_bias=cloud_bias, rows_per_cloud=rows_per_cloud, xyz3=xyz3, w3=w3, out=y)
        return (y,) + tuple(_bn_fwd(y, bn))
    buf = torch.empty(1 + 2 * tiles, C, dtype=torch.float32, device=x.device)
    _run("hsp_gemm_rows_bn_bf16", (_p(x), ops._ld(x), _p(Wc), ops._ld(Wc), K, R, C, _p(b), _p(cloud_bias), int(rows_per_cloud),
                                   _p(xyz3), _p(w3), _p(y), C, _p(buf[0]), _p(buf[1:]), _stream()),
         key=f"M{R}N{C}K{K}bn", abytes=2 * (R + C) * K + 4 * R * C, aflops=2 * R * C * K)
    return (y,) + ops._bn_fwd_raw(y, _bn_state(bn), True, BF16, (buf[1:], tiles, buf[0]))


def _bn_bwd(y, da, gamma, beta, mean, invstd):
    """(bf16 gradient of y, d gamma, d beta) of relu(bn(y)) under train-mode statistics"""
    if mean is None:
        raise HspError("bf16 heads: no backward through an eval-mode BatchNorm")
    return ops._bn_bwd_raw(y, _b(da, "bn_relu.grad"), gamma, beta, mean, invstd, True)


def _xyz_moments(g2, xyz, B):
    """(Cout, 3) = g^T xyz over all rows: the per-cloud coordinate moments of g (one pass, hsp_colsum_rows_xyz_bf16) summed over
    the B clouds -- the xyz columns' block of a weight gradient, no product"""
    R, C = g2.shape
    mom = ops.colsum_rows_xyz(g2.view(B, R // B, C), xyz)
    return mom, mom[:, C:].sum(dim=0).view(3, C).t()


class _DenseBN(torch.autograd.Function):
    """relu(bn(x W^T + b)) over bf16 point rows x (R, K) (rows may sit on a wider pitch: feat)"""

    @staticmethod
    def forward(ctx, bn, x, w, b, gamma, beta):
        x = x if (x.dtype == BF16 and x.is_cuda and x.dim() == 2 and x.stride(1) == 1) else _b(x, "dense_bn.x")
        Wc, _ = copies_of(w)
        y, a, mean, invstd = _product_bn(x, Wc, b, bn, w.shape[0])
        ctx.save_for_backward(x, w, y, gamma, beta, mean, invstd)
        ctx.has_bias = b is not None
        return a

    @staticmethod
    def backward(ctx, da):
        x, w, y, gamma, beta, mean, invstd = ctx.saved_tensors
        g, dg, db = _bn_bwd(y, da, gamma, beta, mean, invstd)
        gx = None
        if ctx.needs_input_grad[1]:
            _, WT = copies_of(w)
            gx = ops.gemm_rows(g, WT)
        gwt, gb = ops.wgrad(x, g, colsum=True)                     # (K, Cout) = dW^T, column sums of g = db
        return None, gx, gwt.t(), (gb if ctx.has_bias else None), dg, db


class _CloudCatBN(torch.autograd.Function):
    """relu(bn(F.linear(cat[fg over each cloud's rows, x, xyz], W, b))) -- the face head's first layer (FaceRecon.py:113-117) as
    ``ops._CloudCatLinear`` forms it (f_global's columns are an fp32 per-cloud bias, the coordinates ride in the epilogue as
    xyz3 . w3: they never pass through bf16), x bf16 (R, Cx)"""

    @staticmethod
    def forward(ctx, bn, fg, x, xyz, W, b, gamma, beta):
        B, Cg = fg.shape
        R, Cx = x.shape
        N = R // B
        x = _b(x, "cloud_cat.x")
        t = ops.gemm_own(fg, W[:, :Cg], False)                  # (B, Cout) fp32: one small launch
        if b is not None:
            t = t + b
        Wc, _ = copies_of(W[:, Cg:Cg + Cx])
        y, a, mean, invstd = _product_bn(x, Wc, None, bn, W.shape[0], cloud_bias=t.contiguous(), rows_per_cloud=N,
                                         xyz3=xyz.reshape(R, 3), w3=W[:, Cg + Cx:].contiguous())
        ctx.save_for_backward(fg, x, xyz, W, y, gamma, beta, mean, invstd)
        ctx.has_bias = b is not None
        return a

    @staticmethod
    def backward(ctx, da):
        fg, x, xyz, W, y, gamma, beta, mean, invstd = ctx.saved_tensors
        B, Cg = fg.shape
        R, Cx = x.shape
        g, dg, db = _bn_bwd(y, da, gamma, beta, mean, invstd)
        Cout = g.shape[1]
        mom, gxyz = _xyz_moments(g, xyz, B)                       # per-cloud column sums of g in mom[:, :Cout]
        gt = mom[:, :Cout]
        gW = torch.empty(Cout, Cg + Cx + 3, dtype=torch.float32, device=g.device)
        ops._tiny_tn(gt, fg, gW[:, :Cg])                          # the f_global block of dW
        gW[:, Cg + Cx:] = gxyz
        g_fg = ops.gemm_own(gt.contiguous(), W[:, :Cg], True) if ctx.needs_input_grad[1] else None
        gx = None
        if ctx.needs_input_grad[2]:
            _, WT = copies_of(W[:, Cg:Cg + Cx])
            gx = ops.gemm_rows(g, WT)
        gW[:, Cg:Cg + Cx] = ops._wgrad_now(x, g).t()
        return None, g_fg, gx, None, gW, (gt.sum(0) if ctx.has_bias else None), dg, db


class _FanBN(torch.autograd.Function):
    """relu(bn_i(x W_i^T + b_i)) for the layers that read feat's rows (the first layers of the three pose heads -- the translation
    head's on cat[x, xyz], its coordinate columns in the epilogue -- and of the reconstruction block).  Backward: the input gradient
    is the sum of the members' g_i W_i, carried in fp32 over products of two sources each (hsp_gemm_rows_bf16 with an fp32 result,
    then hsp_gemm_rows_acc_bf16) and rounded to bf16 ONCE by the last; every weight gradient from the ragged bf16 kernel."""

    @staticmethod
    def forward(ctx, bns, x, xyz, *flat):
        R, K = x.shape
        outs, saved = [], []
        for i, bn in enumerate(bns):
            w, b, gamma, beta = flat[4 * i:4 * i + 4]
            Wc, _ = copies_of(w[:, :K])
            if w.shape[1] == K:
                y, a, mean, invstd = _product_bn(x, Wc, b, bn, w.shape[0])
            else:                                              # cat[x, xyz]: the K = 3 coordinate product in the epilogue
                y, a, mean, invstd = _product_bn(x, Wc, b, bn, w.shape[0], xyz3=xyz.reshape(R, 3), w3=w[:, K:].contiguous())
            outs.append(a)
            saved += [y, mean, invstd]
        ctx.save_for_backward(x, xyz, *flat, *saved)
        ctx.n = len(bns)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *das):
        x, xyz = ctx.saved_tensors[:2]
        n = ctx.n
        flat = ctx.saved_tensors[2:2 + 4 * n]
        saved = ctx.saved_tensors[2 + 4 * n:]
        R, K = x.shape
        gs, grads = [], []
        for i in range(n):
            w, b, gamma, beta = flat[4 * i:4 * i + 4]
            y, mean, invstd = saved[3 * i:3 * i + 3]
            da = das[i] if das[i] is not None else torch.zeros(R, w.shape[0], dtype=BF16, device=x.device)
            g, dg, db = _bn_bwd(y, da, gamma, beta, mean, invstd)
            gs.append((g, copies_of(w[:, :K])[1]))
            if w.shape[1] == K:
                gwt, gb = ops.wgrad(x, g, colsum=True)
                gw = gwt.t()
            else:
                gwt, gb = ops._wgrad_now(x, g, colsum=True)
                gw = torch.empty_like(w)
                gw[:, :K] = gwt.t()
                gw[:, K:] = _xyz_moments(g, xyz, xyz.shape[0])[1]
            grads += [gw, gb if b is not None else None, dg, db]
        gx = None
        if ctx.needs_input_grad[1]:
            # gx = sum_i g_i W_i: pairs of products, the running sum in fp32, ONE rounding to bf16 at the last launch
            gx = torch.empty(R, K, dtype=BF16, device=x.device)
            pairs = [gs[j:j + 2] for j in range(0, n, 2)]
            acc = None
            for j, pr in enumerate(pairs):
                last = j == len(pairs) - 1
                out = gx if last else (acc if acc is not None else torch.empty(R, K, dtype=torch.float32, device=x.device))
                (g1, w1), (g2, w2) = pr[0], (pr[1] if len(pr) > 1 else (None, None))
                if acc is None:
                    ops.gemm_rows(g1, w1, False, g2, w2, False, out=out)
                else:
                    gemm_rows_acc(g1, w1, g2, w2, acc, out)
                acc = out
        return (None, gx, None, *grads)


def gemm_rows_acc(A1, B1, A2, B2, resid, out):
    """out = A1 B1^T (+ A2 B2^T) + resid for bf16 rows / (N,K) bf16 weights and an fp32 ``resid``; out fp32 or bf16
    (hsp_gemm_rows_acc_bf16).  out may be resid itself."""
    M, N, K1, K2, flops, _ = ops._gemm_dims(A1, B1, False, A2)
    for t_ in (A1, B1, A2, B2):
        if t_ is not None and (t_.dtype != BF16 or not t_.is_cuda):
            raise HspError("gemm_rows_acc: bf16 GPU operands")
    if resid.dtype != torch.float32 or resid.shape != (M, N) or out.shape != (M, N):
        raise HspError("gemm_rows_acc: fp32 resid and out of shape (M, N)")
    wsb = lib().hsp_gemm_rows_workspace_bytes(M, N, K1, K2, 2)
    ws = _ws(wsb, A1.device) if wsb else None
    _run("hsp_gemm_rows_acc_bf16", (*ops._gemm_sources(A1, ops._w(B1), K1, A2, ops._w(B2), K2), M, N, _p(resid), ops._ld(resid), _p(out),
                                    ops._ld(out), 1 if out.dtype == torch.float32 else 0, _p(ws), wsb, _stream()),
         key=f"M{M}N{N}K{K1}+{K2}acc", abytes=2 * (M + N) * (K1 + K2) + 4 * M * N + ops._es(out) * M * N, aflops=flops)
    return out


class _LinearBf16(torch.autograd.Function):
    """y = x W^T + b for bf16 rows x (R, K) -> fp32 y: the heads' last layers (recon 3-wide, face 30-wide: FaceRecon.py:48,68)"""

    @staticmethod
    def forward(ctx, x, w, b):
        x = _b(x, "linear_rows.x")
        Wc, _ = copies_of(w)
        y = ops.gemm_rows(x, Wc, bias=b, out=torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device))
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = _req(g, torch.float32, "linear_rows.grad")
        R, Cout = g.shape
        gx = None
        if ctx.needs_input_grad[0]:
            # a K = Cout <= 30 product (no bf16 MFMA shape): fp32 on the hand-written kernel, rounded once to bf16
            gx = ops.gemm_rows(g, w, True).to(BF16)
        gwt = ops._wgrad_thin(x, g, now=True)                           # (g rounded to bf16 on the padded columns)
        gb = ops.colsum_rows(g.view(1, R, Cout)).view(Cout) if ctx.has_bias else None      # (from the fp32 g)
        return gx, gwt.t(), gb


def dense_bn(x, w, b, bn):
    """relu(bn(x W^T + b)) for bf16 rows x (R, K) -> bf16 rows (one node; ``w``: the fp32 master as (Cout, K))"""
    return _DenseBN.apply(bn, x, w, b, bn.weight, bn.bias)


def cloud_cat_bn(fg, x, xyz, W, b, bn):
    """relu(bn(F.linear(cat[fg (B, Cg) over each cloud, x (R, Cx) bf16, xyz (B, N, 3)], W, b))) -> bf16 rows"""
    return _CloudCatBN.apply(bn, fg, x, xyz, W, b, bn.weight, bn.bias)


def fan_bn(x, xyz, layers):
    """[relu(bn_i(x or cat[x, xyz] W_i^T + b_i)) for (W_i, b_i, bn_i) in layers] for bf16 rows x (R, K) that every layer reads;
    a weight with K + 3 columns reads cat[x, xyz]"""
    flat = []
    for w, b, bn in layers:
        flat += [w, b, bn.weight, bn.bias]
    return _FanBN.apply(tuple(bn for _, _, bn in layers), x, xyz, *flat)


def linear_rows(x2, w, b=None):
    return _LinearBf16.apply(x2, w, b)
