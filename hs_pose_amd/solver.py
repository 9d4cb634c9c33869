"""Training-driver pieces: the Ranger optimizer as ONE fused device step, gradient-norm clipping without a
host round trip, and the flat-and-anneal learning-rate schedule.

Mirrors (same names, arguments and state_dict layout):
  Ranger                         tools/torch_utils/solver/ranger2020.py:44-246
  flat_and_anneal_lr_scheduler   tools/torch_utils/solver/lr_scheduler.py:177-263
  build_optimizer, build_lr_rate tools/training_utils.py:13-56
  clip_grad_norm_                torch.nn.utils.clip_grad_norm_ as used in engine/train.py:99,104

The reference's ``Ranger.step`` walks the parameter tensors in Python (~10 elementwise launches each).  Here
the parameters of a group are re-seated as views of one flat fp32 buffer, and so are their gradients and the
three state tensors; ``step()`` is a single ``hsp_ranger_step`` launch per group (csrc/optim.hip) driven by a
device table of rows.  ``state_dict()`` still holds per-parameter ``step / exp_avg / exp_avg_sq / slow_buffer``
entries (views), so checkpoints written by either implementation load into the other.
"""
import ctypes
import math

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import ops
from ._lib import (STEP_ADAPTIVE, STEP_CTL_APPLIED, STEP_CTL_APPLY, STEP_CTL_ARMED, STEP_CTL_EXHAUSTED, STEP_CTL_FIRST,
                   STEP_CTL_INDEX, STEP_CTL_MICRO, STEP_CTL_PENDING, STEP_CTL_REPLAYS, STEP_CTL_SKIPPED_NAN,
                   STEP_CTL_SKIPPED_NO_ITEM, STEP_CTL_SLOTS, STEP_CTL_TAKE, STEP_FILL_SLOW, STEP_LOOKAHEAD, HspError,
                   HspRowDesc, lib)
from .config import FLAGS

_ROW_CHUNK = 4096          # 1-D tensors are cut into rows of at most this many elements


class _FlatGroup:
    """flat storage of one param group: parameters, gradients, exp_avg, exp_avg_sq, slow weights + the row table."""

    def __init__(self, params):
        self.params = [p for p in params]
        if not self.params:
            raise HspError("Ranger: empty parameter group")
        dev = self.params[0].device
        for p in self.params:
            if not p.is_cuda or p.dtype != torch.float32 or p.device != dev:
                raise HspError("Ranger: parameters must be fp32 tensors on one GPU (hs_pose_amd has no CPU path)")
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 3) & ~3                      # 16-byte aligned starts
        self.offsets, self.total = offs, total
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_s = torch.zeros(total, dtype=torch.float32, device=dev)
        rows = []
        for p, o in zip(self.params, offs):
            n = p.numel()
            self.view(self.flat_p, p, o).copy_(p.data)
            p.data = self.view(self.flat_p, p, o)              # the parameter now lives in the flat buffer
            g = self.view(self.flat_g, p, o)
            if p.grad is not None:
                g.copy_(p.grad)
            p.grad = g                                         # autograd accumulates in place into the flat buffer
            if p.dim() > 1:
                rl = n // p.shape[0]
                rows += [(o + r * rl, rl, 1) for r in range(p.shape[0])]
            else:
                rows += [(o + c, min(_ROW_CHUNK, n - c), 0) for c in range(0, n, _ROW_CHUNK)]
        # slow_buffer is filled from the weights at the FIRST step(), like the reference creates it lazily
        # (ranger2020.py:168-170): weights loaded between construction and the first step must be what Lookahead
        # interpolates towards, not the random init that was live when the optimizer was built
        self.slow_ready = False
        self.rows_host = rows                                  # (offset, len, gc) in HspRowDesc's field order
        self.rows = self._upload(rows)
        self.nrows = len(rows)
        self.flat_f = None                                     # the FRESH gradient of a replay (gradient accumulation only)

    def fresh(self):
        """the second flat gradient buffer, made when gradient accumulation is first asked for: a replay's fresh gradient lands
        here, and ``flat_g`` becomes the accumulator ``hsp_grad_accumulate`` adds it to"""
        if self.flat_f is None:
            self.flat_f = torch.zeros_like(self.flat_g)
        return self.flat_f

    def _upload(self, rows):
        return ops.upload_table((HspRowDesc * len(rows))(*rows), self.flat_p.device)

    @staticmethod
    def view(flat, p, off):
        return flat[off:off + p.numel()].view(p.shape)

    def rows_for(self, use_gc, gc_conv_only):
        """row table with the gc flag resolved (conv-only: tensors with more than 3 dims, ranger2020.py:34-36)."""
        if use_gc and not gc_conv_only:
            return self.rows
        key = (use_gc, gc_conv_only)
        cache = self.__dict__.setdefault("_rows_cache", {})
        if key not in cache:
            gc = [use_gc and g for _, _, g in self.rows_host]
            if use_gc:
                i = 0
                for p in self.params:
                    nr = p.shape[0] if p.dim() > 1 else (p.numel() + _ROW_CHUNK - 1) // _ROW_CHUNK
                    if p.dim() <= 3:
                        gc[i:i + nr] = [0] * nr
                    i += nr
            cache[key] = self._upload([(o, n, int(g)) for (o, n, _), g in zip(self.rows_host, gc)])
        return cache[key]


def _radam_step_size(step, beta1, beta2, thresh):
    """(N_sma > threshold, step_size) of ranger2020.py:194-212 (host scalars, cached per step by the reference)."""
    beta2_t = beta2 ** step
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma > thresh:
        ss = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** step)
        return True, ss
    return False, 1.0 / (1 - beta1 ** step)


STEP_ENTRY = np.dtype([("step_lr", "<f4"), ("flags", "<i4")])       # HspStepEntry (include/hsp.h)


def step_table(step0, epoch0, horizon, base_lr, factor, betas, k, n_sma_threshold, fill_slow=False):
    """The host scalars of the next ``horizon`` applied steps of one parameter group, as the ``HspStepEntry`` rows
    ``hsp_ranger_step_gated`` reads (a numpy array of ``STEP_ENTRY``).  Entry ``j`` is the step ``step0 + j + 1`` taken at the
    learning rate ``base_lr * factor(epoch0 + j)`` -- what ``LambdaLR`` holds after ``epoch0 + j`` scheduler steps --:

      step_lr   ``step_size * lr`` by the expressions of ``Ranger.step()`` (``_radam_step_size``, Python doubles), rounded to
                fp32 once: the bits the host path hands ``hsp_ranger_step`` by value
      flags     STEP_ADAPTIVE (N_sma > threshold) | STEP_LOOKAHEAD (step % k == 0) | on entry 0 only, with ``fill_slow``,
                STEP_FILL_SLOW (the slow weights are taken from the weights before that step)

    ``factor`` is the scheduler's own lambda, called here on the host: any schedule works, and the device does no arithmetic
    on the clock at all (a device ``pow`` / ``cos`` would match the host's libm to an ulp only, and the step would stop being the
    host path's bit for bit).  Pure: no device, no optimizer."""
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError(f"step_table: expects horizon >= 1, got {horizon}")
    beta1, beta2 = betas
    out = np.zeros(horizon, dtype=STEP_ENTRY)
    for j in range(horizon):
        step = int(step0) + j + 1
        lr = base_lr * factor(int(epoch0) + j)
        adaptive, step_size = _radam_step_size(step, beta1, beta2, n_sma_threshold)
        out["step_lr"][j] = np.float32(step_size * lr)
        out["flags"][j] = (STEP_ADAPTIVE if adaptive else 0) | (STEP_LOOKAHEAD if step % k == 0 else 0)
    if fill_slow:
        out["flags"][0] |= STEP_FILL_SLOW
    return out


class DeviceClock:
    """The step count, the schedule and the skip decision of a ``Ranger`` kept ON THE DEVICE (``Ranger.device_clock``), so that
    the optimizer launch can be captured in the training step's graph: one ``step_table`` per parameter group, uploaded once,
    and the sixteen-slot control block of include/hsp.h.  ``gate(total)`` issues ``hsp_step_gate`` -- the device decides whether
    this replay's step is applied (NaN loss, no good item, table used up: no) and names the table entry --, ``step()`` one
    ``hsp_ranger_step_gated`` per group.  Neither reads or writes a host counter: ``state[p]['step']``, the scheduler and the
    groups' ``lr`` are current only after ``Ranger.sync_clock()``.

    The block is built UNARMED: the gate then answers "do not apply" and counts nothing, so the warm-up runs of a capture
    execute both kernels and leave parameters, optimizer state and counters as they were.  ``arm()`` uploads armed = 1.

    ``accumulate`` > 1: ``gate`` issues ``hsp_step_gate_accum`` instead, which also keeps ``micro`` -- the reference's
    ``global_step``, starting at ``global_step`` and advancing on every armed replay -- and ``pending``, the micro-batches in the
    accumulator (slots 8-11 of the block); the step is applied on the replays with ``micro % accumulate == 0``.  ``rebuild()``
    leaves ``micro`` and ``pending`` as they stand on the device."""

    COUNTERS = ("applied", "replays", "skipped_nan", "skipped_no_item", "exhausted")

    def __init__(self, optimizer, scheduler, horizon, info=None, accumulate=1, global_step=0):
        self.opt, self.sched, self.info = optimizer, scheduler, info
        self.accumulate = int(accumulate)
        if self.accumulate < 1:
            raise ValueError(f"device_clock: expects accumulate >= 1, got {accumulate}")
        if not 0 <= int(global_step) < 2 ** 31 - 1:
            raise ValueError(f"device_clock: global_step expects a non-negative int32, got {global_step}")
        if horizon is None:
            if scheduler is None or not hasattr(scheduler, "total_iters"):
                raise ValueError("device_clock: horizon=None needs a scheduler that records total_iters "
                                 "(flat_and_anneal_lr_scheduler does); give the number of steps to tabulate")
            horizon = int(scheduler.total_iters) - int(scheduler.last_epoch)
        self.horizon = int(horizon)
        if self.horizon < 1:
            raise ValueError(f"device_clock: expects horizon >= 1, got {self.horizon}")
        if info is not None and (not info.is_cuda or info.dtype != torch.int32 or info.numel() < 1):
            raise ValueError("device_clock: info expects hsp_batch_select's int32 device tensor")
        dev = optimizer._flat[0].flat_p.device
        self.ctl = torch.zeros(STEP_CTL_SLOTS, dtype=torch.int32, device=dev)
        self.tables = [torch.zeros(self.horizon * STEP_ENTRY.itemsize, dtype=torch.uint8, device=dev) for _ in optimizer._flat]
        self.tables_host = None
        self.rebuild()
        if self.accumulate > 1:
            self.set_micro(int(global_step), 0)

    def set_micro(self, micro, pending):
        """``micro`` and ``pending`` as the host gives them (construction, a loaded checkpoint): one small upload"""
        self.ctl[STEP_CTL_MICRO:STEP_CTL_PENDING + 1].copy_(torch.tensor([int(micro), 0, 0, int(pending)], dtype=torch.int32))

    def rebuild(self):
        """tabulate the next ``horizon`` steps from the optimizer's and the scheduler's counts AS THEY STAND ON THE HOST, into
        the same device buffers (a captured graph keeps reading them), and zero the device counters; the armed flag stays"""
        opt, sch = self.opt, self.sched
        self.epoch0 = int(sch.last_epoch) if sch is not None else 0
        self.sched_count0 = int(getattr(sch, "_step_count", 0)) if sch is not None else 0
        self.step0, self.slow_ready0, self.tables_host = [], [], []
        for g, (group, fg) in enumerate(zip(opt.param_groups, opt._flat)):
            step0 = int(opt.state[fg.params[0]]["step"])
            base_lr, factor = (sch.base_lrs[g], sch.lr_lambdas[g]) if sch is not None else (group["lr"], lambda x: 1.0)
            tab = step_table(step0, self.epoch0, self.horizon, base_lr, factor, group["betas"], group["k"],
                             opt.N_sma_threshhold, fill_slow=not fg.slow_ready)
            self.tables[g].copy_(torch.from_numpy(tab.view(np.uint8)))
            self.step0.append(step0)
            self.slow_ready0.append(bool(fg.slow_ready))
            self.tables_host.append(tab)
        if self.accumulate > 1:                                # micro and pending go on from where they are
            self.ctl[1:STEP_CTL_MICRO].zero_()
            self.ctl[STEP_CTL_TAKE:STEP_CTL_FIRST + 1].zero_()
        else:
            self.ctl[1:].zero_()

    def arm(self, on=True):
        self.ctl[STEP_CTL_ARMED:STEP_CTL_ARMED + 1].fill_(1 if on else 0)

    def gate(self, total):
        if not total.is_cuda or total.dtype != torch.float32 or total.numel() != 1:
            raise HspError(f"DeviceClock.gate: expects the fp32 total loss on the device, got {total.dtype} {tuple(total.shape)}")
        if self.accumulate > 1:
            ops._run("hsp_step_gate_accum", (ops._p(total), ops._p(self.info), ops._p(self.ctl), self.horizon, self.accumulate,
                                             ops._stream()))
            return
        ops._run("hsp_step_gate", (ops._p(total), ops._p(self.info), ops._p(self.ctl), self.horizon, ops._stream()))

    def step(self):
        opt = self.opt
        for group, fg, table in zip(opt.param_groups, opt._flat, self.tables):
            opt._collect_grads(fg)
            beta1, beta2 = group["betas"]
            rows = fg.rows_for(opt.use_gc, opt.gc_conv_only)
            ops._run("hsp_ranger_step_gated",
                     (ops._p(fg.flat_p), ops._p(fg.flat_g), ops._p(fg.flat_m), ops._p(fg.flat_v), ops._p(fg.flat_s),
                      ops._p(rows), fg.nrows, beta1, beta2, group["eps"], group["weight_decay"], opt.alpha,
                      int(not opt.gc_loc), ops._p(opt._gnorm_sq), opt._max_norm, ops._p(table), ops._p(self.ctl),
                      self.horizon, ops._stream()),
                     key=f"n{fg.total}", abytes=fg.total * 44)
        opt._gnorm_sq = None

    def read(self):
        """the control block, one small device->host copy (a wait): {'armed', 'apply', 'index', 'applied', 'replays',
        'skipped_nan', 'skipped_no_item', 'exhausted'} and the accumulation slots {'micro', 'take', 'first', 'pending'}, which
        stay 0 unless ``accumulate`` > 1"""
        c = self.ctl.cpu().tolist()
        return dict(armed=c[STEP_CTL_ARMED], apply=c[STEP_CTL_APPLY], index=c[STEP_CTL_INDEX], applied=c[STEP_CTL_APPLIED],
                    replays=c[STEP_CTL_REPLAYS], skipped_nan=c[STEP_CTL_SKIPPED_NAN],
                    skipped_no_item=c[STEP_CTL_SKIPPED_NO_ITEM], exhausted=c[STEP_CTL_EXHAUSTED],
                    micro=c[STEP_CTL_MICRO], take=c[STEP_CTL_TAKE], first=c[STEP_CTL_FIRST], pending=c[STEP_CTL_PENDING])

    def applied_last(self):
        """the device's decision on the last replay (a wait)"""
        return bool(int(self.ctl[STEP_CTL_APPLY]))

    def taken_last(self):
        """``accumulate`` > 1: whether the last replay's gradient entered the accumulator (a wait)"""
        return bool(int(self.ctl[STEP_CTL_TAKE]))


class GradAccumulation:
    """Gradient accumulation on a ``Ranger``'s flat buffers (``Ranger.accumulation``; engine/train.py:99-114).  ``flat_g`` is the
    ACCUMULATOR -- what ``hsp_ranger_step`` / ``hsp_ranger_step_gated`` read --, ``flat_f`` (``_FlatGroup.fresh``) receives a
    replay's fresh gradient, ``norm_sq`` is the device scalar ``hsp_grad_accumulate`` keeps beside the accumulator: its squared
    norm, from which the next take, or the step, derives the clip coefficient.  WHILE ``pending == 0`` THE CONTENTS OF THE
    ACCUMULATOR AND OF ``norm_sq`` MEAN NOTHING: nothing clears them after a step, the next take starts afresh.

    ``micro`` (the reference's ``global_step``) and ``pending`` (micro-batches in the accumulator) live on the device when a
    ``DeviceClock`` decides (``clock``), else here on the host.  One parameter group only."""

    def __init__(self, optimizer, accumulate, global_step=0, max_norm=5, clock=None):
        if len(optimizer._flat) != 1:
            raise HspError("gradient accumulation on the flat buffers is built for one parameter group (HSPose.build_params' one)")
        self.opt, self.clock = optimizer, clock
        self.accumulate, self.max_norm = int(accumulate), float(max_norm)
        self.micro, self.pending = int(global_step), 0
        fg = optimizer._flat[0]
        fg.fresh()
        self.norm_sq = torch.zeros(1, dtype=torch.float32, device=fg.flat_g.device)
        self.ws_bytes = lib().hsp_sumsq_workspace_bytes(fg.total)
        self.ws = ops._ws(self.ws_bytes, fg.flat_g.device)

    def take(self, first=None):
        """``hsp_grad_accumulate``: ``flat_g = flat_g * c + flat_f`` (``first``: ``0 + flat_f``) and ``norm_sq`` of the result.
        ``first`` None: gated -- take and first are the device clock's."""
        fg = self.opt._flat[0]
        ctl = self.clock.ctl if first is None else None
        ops._run("hsp_grad_accumulate",
                 (ops._p(fg.flat_g), ops._p(fg.flat_f), fg.total, ops._p(self.norm_sq), self.max_norm, int(bool(first)),
                  ops._p(ctl), ops._p(self.ws), self.ws_bytes, ops._stream()),
                 key=f"n{fg.total}", abytes=fg.total * (8 if first else 12))

    def counts(self):
        """(micro, pending): the host's, or the device clock's (a wait)"""
        if self.clock is None:
            return self.micro, self.pending
        c = self.clock.read()
        return c["micro"], c["pending"]

    def state(self):
        """what a checkpoint needs to resume bit for bit, or None while nothing is pending"""
        micro, pending = self.counts()
        if pending == 0:
            return None
        return dict(micro=micro, pending=pending, grad=self.opt._flat[0].flat_g.detach().clone(),
                    norm_sq=self.norm_sq.detach().clone())

    def load_state(self, st):
        """``state()``'s dict; None (a checkpoint taken with nothing pending): pending = 0, micro stays what the object was
        built with -- like the reference, which derives global_step from the epoch it resumes at"""
        micro, pending = (int(st["micro"]), int(st["pending"])) if st is not None else (self.counts()[0], 0)
        if st is not None:
            self.opt._flat[0].flat_g.copy_(st["grad"])
            self.norm_sq.copy_(st["norm_sq"])
        self.micro, self.pending = micro, pending
        if self.clock is not None:
            self.clock.set_micro(micro, pending)


class Ranger(Optimizer):
    """RAdam + Lookahead + gradient centralisation; arguments and defaults of ranger2020.py:45-58."""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5,
                 weight_decay=0, use_gc=True, gc_conv_only=False, gc_loc=True):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold,
                        eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha, self.k = alpha, k
        self.gc_loc, self.use_gc, self.gc_conv_only = gc_loc, use_gc, gc_conv_only
        self._flat = [_FlatGroup(g["params"]) for g in self.param_groups]
        self._gnorm_sq = None            # device scalar written by clip_grad_norm_, consumed by the next step()
        self._max_norm = 0.0
        self._clock = None               # a DeviceClock (device_clock()): the step count then lives on the device
        self._accum = None               # a GradAccumulation (accumulation()): flat_g is then the accumulator
        for fg in self._flat:
            for p, o in zip(fg.params, fg.offsets):
                self.state[p] = dict(step=0, exp_avg=fg.view(fg.flat_m, p, o), exp_avg_sq=fg.view(fg.flat_v, p, o),
                                     slow_buffer=fg.view(fg.flat_s, p, o))

    # -- gradients -------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        """zero the flat gradient buffers (one memset per group); the .grad views stay in place."""
        for fg in self._flat:
            fg.flat_g.zero_()
            for p, o in zip(fg.params, fg.offsets):
                if p.grad is None or p.grad.data_ptr() != fg.flat_g.data_ptr() + 4 * o:
                    p.grad = fg.view(fg.flat_g, p, o)

    def _collect_grads(self, fg):
        """a backward that REPLACED .grad (first accumulation into a None grad) is copied back into the flat buffer."""
        for p, o in zip(fg.params, fg.offsets):
            if p.grad is None:
                raise HspError("Ranger: every parameter of a group needs a gradient (fused step)")
            if p.grad.data_ptr() != fg.flat_g.data_ptr() + 4 * o:
                v = fg.view(fg.flat_g, p, o)
                v.copy_(p.grad)
                p.grad = v

    def sync_grads(self):
        """make the flat gradient buffers current: a backward that replaced a ``.grad`` (first accumulation into a None
        grad) is copied back into its flat view.  Call before reading ``flat_g`` directly (data-parallel all-reduce)."""
        for fg in self._flat:
            self._collect_grads(fg)

    def scale_grads_by_clip_(self):
        """apply the pending clip coefficient to the gradients IN PLACE now (instead of inside the next step()): what the
        reference's clip_grad_norm_ does on iterations that accumulate without stepping (engine/train.py:103-104).
        Device-side, no host synchronisation."""
        if self._gnorm_sq is None:
            return
        coef = torch.clamp(self._max_norm / (self._gnorm_sq.sqrt() + 1e-6), max=1.0)
        for fg in self._flat:
            fg.flat_g.mul_(coef)
        self._gnorm_sq = None

    def clip_grad_norm_(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(all parameters, max_norm) (engine/train.py:99): the squared norm is reduced
        on the device and the coefficient min(1, max_norm / (norm + 1e-6)) is applied INSIDE the next step() --
        no host synchronisation.  Returns the (device) total norm."""
        L = lib()
        parts = []
        for fg in self._flat:
            self._collect_grads(fg)
            out = torch.empty(1, dtype=torch.float32, device=fg.flat_g.device)
            wsb = L.hsp_sumsq_workspace_bytes(fg.total)
            ws = ops._ws(wsb, fg.flat_g.device)
            ops._run("hsp_sumsq_f32", (ops._p(fg.flat_g), fg.total, ops._p(out), ops._p(ws), wsb, ops._stream()),
                     key=f"n{fg.total}", abytes=4 * fg.total)
            parts.append(out)
        self._gnorm_sq = parts[0] if len(parts) == 1 else torch.stack(parts).sum(dim=0)
        self._max_norm = float(max_norm)
        return self._gnorm_sq.sqrt()

    # -- the step --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if self._clock is not None:
            raise HspError("Ranger.step(): a device clock is attached (device_clock()): the step is DeviceClock.step(), gated on "
                           "the device, and a host step would leave the device's count behind")
        for group, fg in zip(self.param_groups, self._flat):
            self._collect_grads(fg)
            if not fg.slow_ready:                                  # first step of this group: slow weights = weights now
                fg.flat_s.copy_(fg.flat_p)
                fg.slow_ready = True
            st0 = self.state[fg.params[0]]
            step = int(st0["step"]) + 1
            beta1, beta2 = group["betas"]
            adaptive, step_size = _radam_step_size(step, beta1, beta2, self.N_sma_threshhold)
            look = step % group["k"] == 0
            rows = fg.rows_for(self.use_gc, self.gc_conv_only)
            ops._run("hsp_ranger_step",
                     (ops._p(fg.flat_p), ops._p(fg.flat_g), ops._p(fg.flat_m), ops._p(fg.flat_v), ops._p(fg.flat_s),
                      ops._p(rows), fg.nrows, beta1, beta2, group["eps"], group["weight_decay"],
                      step_size * group["lr"], int(adaptive), int(look), self.alpha, int(not self.gc_loc),
                      ops._p(self._gnorm_sq), self._max_norm, ops._stream()),
                     key=f"n{fg.total}", abytes=fg.total * (44 + (8 if look else 0)))
            for p in fg.params:
                self.state[p]["step"] = step
        self._gnorm_sq = None
        return loss

    # -- the step clock on the device ------------------------------------------------------------------------
    def device_clock(self, scheduler=None, horizon=None, info=None, accumulate=1, global_step=0):
        """Attach and return a ``DeviceClock``: the next ``horizon`` steps tabulated from this optimizer's step counts and
        ``scheduler``'s epoch (a ``LambdaLR``; None: the groups' ``lr`` as they stand), and an unarmed control block.
        ``horizon`` None: the rest of the schedule, ``scheduler.total_iters - scheduler.last_epoch``.  ``info``:
        ``hsp_batch_select``'s device tensor when the gate is to skip a batch without a good item.

        FROM HERE ON ``step()`` raises and ``scheduler.step()`` is never to be called: the counts advance on the device, and
        ``state[p]['step']``, ``scheduler.last_epoch`` and the groups' ``lr`` are current only after ``sync_clock()``
        (``state_dict()`` and ``TrainDriver.checkpoint()`` call it).  Not offered with more than one rank: the ranks' gates could
        disagree.  ``accumulate`` > 1: the clock also counts the micro-batches from ``global_step`` on and applies the step when
        ``micro % accumulate == 0`` (``DeviceClock``); ``sync_clock()`` then reports ``micro`` and ``pending`` too."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise HspError("Ranger.device_clock: not offered with more than one rank (each rank's gate would decide on its own loss)")
        if scheduler is not None and not hasattr(scheduler, "lr_lambdas"):
            raise ValueError("Ranger.device_clock: expects a LambdaLR scheduler (its lr_lambdas are tabulated) or None")
        if self._clock is not None:                        # a new clock starts from where the old one got to
            self.sync_clock()
        self._clock = DeviceClock(self, scheduler, horizon, info, accumulate, global_step)
        return self._clock

    # -- gradient accumulation -------------------------------------------------------------------------------
    def accumulation(self, accumulate, global_step=0, max_norm=5, clock=None):
        """Attach and return a ``GradAccumulation``: from here on ``flat_g`` is the accumulator and a fresh gradient belongs in
        ``_flat[0].flat_f``.  ``clock``: the ``DeviceClock`` (built with the same ``accumulate``) whose gate decides; None: the
        host counts ``micro`` and ``pending``."""
        if int(accumulate) < 1:
            raise ValueError(f"Ranger.accumulation: expects accumulate >= 1, got {accumulate}")
        self._accum = GradAccumulation(self, accumulate, global_step, max_norm, clock)
        return self._accum

    def accumulated_grads(self):
        """The accumulated gradient of every parameter as ``p.grad`` would hold it in the eager driver, as fresh tensors: the
        accumulator with the pending clip coefficient applied (the clip of an accumulate-only slot is deferred into the next
        take), zeros while nothing is pending.  A wait when the counts live on the device."""
        acc = getattr(self, "_accum", None)
        if acc is None:
            raise HspError("Ranger.accumulated_grads: no gradient accumulation attached (accumulation())")
        fg = self._flat[0]
        if acc.counts()[1] == 0:
            flat = torch.zeros_like(fg.flat_g)
        else:
            coef = torch.clamp(torch.full_like(acc.norm_sq, acc.max_norm) / (acc.norm_sq.sqrt() + 1e-6), max=1.0)
            flat = fg.flat_g * coef
        return [fg.view(flat, p, o).clone() for p, o in zip(fg.params, fg.offsets)]

    def sync_clock(self):
        """One small device->host copy of the control block (a wait); the host's mirror is set to what the host-driven path would
        hold after the ``applied`` steps the device has taken since the tables were built: every ``state[p]['step']``, the groups'
        ``slow_ready``, ``scheduler.last_epoch`` / ``_last_lr`` / ``_step_count`` and each group's ``lr``.  Returns the counters."""
        ck = self._clock
        if ck is None:
            raise HspError("Ranger.sync_clock: no device clock attached")
        c = ck.read()
        n = c["applied"]
        for g, (group, fg) in enumerate(zip(self.param_groups, self._flat)):
            for p in fg.params:
                self.state[p]["step"] = ck.step0[g] + n
            fg.slow_ready = ck.slow_ready0[g] or n > 0
        sch = ck.sched
        if sch is not None:
            sch.last_epoch = ck.epoch0 + n
            sch._step_count = ck.sched_count0 + n
            lrs = [base * lmbda(sch.last_epoch) for base, lmbda in zip(sch.base_lrs, sch.lr_lambdas)]      # LambdaLR.get_lr
            for group, lr in zip(self.param_groups, lrs):
                group["lr"] = lr
            sch._last_lr = lrs
        return c

    # -- checkpoints -----------------------------------------------------------------------------------------
    def state_dict(self):
        if self._clock is not None:
            self.sync_clock()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """accepts checkpoints of the reference Ranger (per-parameter tensors): values are copied into the flat state.  With a
        device clock attached its tables are rebuilt from the loaded counts and the device counters zeroed -- from the
        scheduler AS IT STANDS: one loaded afterwards needs ``clock.rebuild()`` (``TrainDriver.load_checkpoint`` does it)."""
        super().load_state_dict(state_dict)
        for fg in self._flat:
            # a checkpoint written after >= 1 step carries every slow_buffer; one without them -- or one this optimizer wrote BEFORE
            # its first step, whose slow_buffer views exist but still hold zeros -- leaves the lazy fill armed
            fg.slow_ready = all("slow_buffer" in self.state[p] and int(self.state[p].get("step", 0)) > 0 for p in fg.params)
            for p, o in zip(fg.params, fg.offsets):
                st = self.state[p]
                for name, flat in (("exp_avg", fg.flat_m), ("exp_avg_sq", fg.flat_v), ("slow_buffer", fg.flat_s)):
                    v = fg.view(flat, p, o)
                    if name in st:
                        v.copy_(st[name])
                    st[name] = v
                st["step"] = int(st.get("step", 0))
        if self._clock is not None:
            self._clock.rebuild()


def clip_grad_norm_(optimizer, max_norm):
    """drop-in for ``torch.nn.utils.clip_grad_norm_(network.parameters(), max_norm)`` in the train loop when the
    optimizer is the fused Ranger (the scaling itself happens in ``optimizer.step()``)."""
    return optimizer.clip_grad_norm_(max_norm)


# ------------------------------------------------------------------------------------------------------------
# learning-rate schedule
# ------------------------------------------------------------------------------------------------------------

def flat_and_anneal_factor(x, total_iters, warmup_iters=0, warmup_factor=0.1, warmup_method="linear", anneal_point=0.72,
                           anneal_method="cosine", target_lr_factor=0, poly_power=1.0, step_gamma=0.1,
                           steps=(2 / 3.0, 8 / 9.0)):
    """lr factor at iteration x (lr_scheduler.py:219-261): warm-up, flat, then anneal from anneal_point*total_iters."""
    from bisect import bisect_right
    anneal_start = (steps[0] if anneal_method == "step" else anneal_point) * total_iters
    if x < warmup_iters:
        if warmup_method == "linear":
            a = float(x) / warmup_iters
            return warmup_factor * (1 - a) + a
        return warmup_factor
    if x >= anneal_start:
        if anneal_method == "step":
            return step_gamma ** bisect_right([s * total_iters for s in steps], float(x))
        frac = (float(x) - anneal_start) / (total_iters - anneal_start)
        if anneal_method == "cosine":
            return target_lr_factor + 0.5 * (1 - target_lr_factor) * (1 + math.cos(math.pi * frac))
        if anneal_method == "linear":
            return target_lr_factor + (1 - target_lr_factor) * (total_iters - float(x)) / (total_iters - anneal_start)
        if anneal_method == "poly":
            return target_lr_factor + (1 - target_lr_factor) * ((total_iters - float(x)) / (total_iters - anneal_start)) ** poly_power
        if anneal_method == "exp":
            return max(target_lr_factor, 5e-3) ** frac
        return 1
    return 1


def flat_and_anneal_lr_scheduler(optimizer, total_iters, warmup_iters=0, warmup_factor=0.1, warmup_method="linear",
                                 anneal_point=0.72, anneal_method="cosine", target_lr_factor=0, poly_power=1.0,
                                 step_gamma=0.1, steps=(2 / 3.0, 8 / 9.0)):
    if warmup_method not in ("constant", "linear"):
        raise ValueError("Only 'constant' or 'linear' warmup_method accepted, got {}".format(warmup_method))
    if anneal_method not in ("cosine", "linear", "poly", "exp", "step", "none"):
        raise ValueError("Only 'cosine', 'linear', 'poly', 'exp', 'step' or 'none' anneal_method accepted, got {}".format(anneal_method))
    if anneal_method != "step" and not 0 <= anneal_point <= 1:
        raise ValueError("anneal_point should be in [0,1], got {}".format(anneal_point))
    scheduler = torch.optim.lr_scheduler.LambdaLR(
        optimizer, lambda x: flat_and_anneal_factor(x, total_iters, warmup_iters, warmup_factor, warmup_method, anneal_point,
                                                    anneal_method, target_lr_factor, poly_power, step_gamma, steps))
    scheduler.total_iters = total_iters            # (the length of the schedule: the default horizon of Ranger.device_clock)
    return scheduler


def build_optimizer(params):
    """tools/training_utils.py:38-56 with the reference's flag defaults: Ranger(lr=FLAGS.lr, weight_decay=0)."""
    kind = getattr(FLAGS, "optimizer_type", "Ranger")
    if kind != "Ranger":
        raise NotImplementedError(f"optimizer_type {kind}: only Ranger (the reference's default) is built")
    groups = list(params)
    return Ranger(groups, lr=float(getattr(FLAGS, "lr", 1e-4)), weight_decay=0)


def build_lr_rate(optimizer, total_iters):
    """tools/training_utils.py:13-35: flat_and_anneal with the flag defaults (warm-up 1000 iters from 0.001, cosine from 72 %)."""
    name = getattr(FLAGS, "lr_scheduler_name", "flat_and_anneal")
    if name != "flat_and_anneal":
        raise NotImplementedError(f"lr_scheduler_name {name}: only flat_and_anneal (the reference's default) is built")
    return flat_and_anneal_lr_scheduler(
        optimizer, total_iters, warmup_iters=getattr(FLAGS, "warmup_iters", 1000),
        warmup_factor=getattr(FLAGS, "warmup_factor", 0.001), warmup_method=getattr(FLAGS, "warmup_method", "linear"),
        anneal_point=getattr(FLAGS, "anneal_point", 0.72), anneal_method=getattr(FLAGS, "anneal_method", "cosine"),
        target_lr_factor=0, poly_power=getattr(FLAGS, "poly_power", 1.0), step_gamma=getattr(FLAGS, "gamma", 0.1))
