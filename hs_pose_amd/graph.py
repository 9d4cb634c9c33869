"""hipGraph capture of the launch-bound steps of the path.

* ``GraphedStep``       -- one HS-stack training step (zero_grad, forward, backward): what ``bench.py`` times.  At B=16,
  N=1028 it is ~185 launches of 5-100 us; issued eagerly from Python the GPU idles between them.  Optionally packs the
  gradients into one flat buffer for the data-parallel exchange, or splits the step in two graphs so that the first
  all-reduce overlaps the rest of the backward.
* ``GraphedNetwork``    -- ``posenet`` forward / backward of the FULL model as two graphs behind one autograd node, for
  ``engine/train.py``'s step (losses and optimizer stay eager).
* ``GraphedInference``  -- the timed body of ``evaluation/evaluate.py`` (eval forward + generate_RT).
* ``GraphedTrainStep``  -- the whole training step incl. augmentation, losses, backward and the gradient norm as ONE graph,
  followed by one fused optimizer launch from the host (``apply='host'``, the default: what ``bench.py`` times as unit U3) or
  with the optimizer launch, the schedule and the NaN skip inside the graph too (``apply='graph'``: a replay is the step).
* ``capture_scope``     -- how all four are captured (timer off, state rolled back, warm-up on a side stream, ``thread_local``
  capture), stated once with its reasons; the timing scripts under ``tools/`` capture through it too.

Static shapes, static input / gradient buffers.  The only host work of the reference's forward -- the two
``torch.randperm`` draws of the Pool_layers on the CPU default generator (gcn3d.py:243) -- happens BEFORE each replay,
in the same order and on the same generator as the reference, and is uploaded into static index buffers the captured
kernels read.  Under the 'fps' pool sampler (config.FLAGS.pool_sampler / gcn3d.Pool_layer(sampler=...), as it stands when the
object is built) the kept rows are picked INSIDE the captured graph from the clouds in the static input buffers: no draw, no
upload and no index buffers, a replay begins with no host work at all.

Under device draws (``config.FLAGS.step_draws = 'device'`` or ``draws=`` on ``GraphedTrainStep`` / ``GraphedInference``, resolved
when the object is built) the 'random' rows -- and the training step's augmentation draws -- are keyed draws made INSIDE the
captured body (include/hsp.h: "keyed draws of a step"): the body begins with ``hsp_pool_rows_draw`` into the static index
buffers, nothing is drawn or uploaded before a replay, and the owner's one action per replay is ``sampler.advance()``.
``GraphedStep`` and ``GraphedNetwork`` keep the host draws.
"""
import contextlib
import gc
import os

import torch

from . import augment, gcn3d, ops, pc_sample, staging
from .config import FLAGS

def draw_pool_indices(n_points, rate=4, levels=2):
    """consume the CPU default generator exactly like FaceRecon's two Pool_layers (FaceRecon.py:91,96)."""
    out, n = [], n_points
    for _ in range(levels):
        m = int(n / rate)
        out.append(torch.randperm(n)[:m])
        n = m
    return out



def alloc_pool_indices(n_points, device):
    """the static index buffers of the two Pool_layers as views of ONE device buffer (so that both are uploaded by one copy)"""
    n1 = int(n_points / 4)
    n2 = int(n1 / 4)
    flat = torch.empty(n1 + n2, dtype=torch.int32, device=device)
    views = [flat[:n1], flat[n1:]]
    views[0]._hsp_flat = flat
    return views


def pool_index_buffers(module, n_points, device):
    """the static Pool_layer index buffers a captured ``module`` needs: ``alloc_pool_indices`` under the 'random' sampler, None
    under 'fps' (the rows are picked inside the graph)"""
    return None if gcn3d.module_sampler(module) == "fps" else alloc_pool_indices(n_points, device)


def pool_feed(bufs):
    """the scope a captured body runs its forward in: the index buffers fed to the Pool_layers, or nothing to feed (None)"""
    return gcn3d.pool_index_feed(bufs) if bufs is not None else contextlib.nullcontext()


def upload_pool_indices(bufs, n_points):
    """draw the Pool_layer permutations (host generator, reference order) and queue their upload on the current
    stream WITHOUT blocking the host: the copy comes from a ring of pinned staging buffers (hs_pose_amd/staging.py),
    stream-ordered after the previous replay and before the next, so the host can enqueue step i+1 while step i is still
    running.  Buffers made by ``alloc_pool_indices`` travel in ONE copy (a copy kernel per pool cost ~5 us of every step)."""
    if bufs is None:                                     # 'fps' sampler: nothing is drawn on the host
        return
    draws = draw_pool_indices(n_points)
    flat = getattr(bufs[0], "_hsp_flat", None)
    if flat is not None:
        def fill(pinned):
            o = 0
            for idx in draws:
                pinned[o:o + idx.numel()].copy_(idx)
                o += idx.numel()
        staging.upload(fill, flat.shape, torch.int32, flat.device, out=flat)
        return
    for buf, idx in zip(bufs, draws):
        staging.upload(lambda pinned, idx=idx: pinned.copy_(idx), buf.shape, torch.int32, buf.device, out=buf)


def draw_pool_rows(scope, bufs, n_points):
    """device draws: the head of a captured body -- both Pool_layers' rows drawn under the scope's key straight into the static
    index buffers (``alloc_pool_indices``) the body's ``pool_feed`` hands to the layers.  Nothing under host draws (``scope`` is
    None) or the 'fps' sampler (``bufs`` is None)."""
    if scope is not None and bufs is not None:
        ops.pool_rows_draw(scope.key, n_points, 4, 2, out=bufs[0]._hsp_flat)


class _keep_sampler_state:
    """building a captured object runs its body eagerly (the warm-up), and an eager body advances the sampler of its device
    draws: state and device key are put back on exit, so the first replay draws what it would have drawn had nothing been built"""

    def __init__(self, sampler):
        self.sampler = sampler

    def __enter__(self):
        if self.sampler is not None:
            self.state, self.key = self.sampler.get_state(), self.sampler.key.clone()
        return self

    def __exit__(self, *exc):
        if self.sampler is not None:
            self.sampler.set_state(self.state)
            self.sampler.key.copy_(self.key)                 # (the key on the device too: what the last advance() uploaded)
        return False


class _preserve_bn_stats:
    """Warm-up forwards run the live network in train mode on the EXAMPLE batch; without this their BatchNorm
    running_mean / running_var / num_batches_tracked updates would leak into the model (and its checkpoints) although
    no training step has happened.  The buffers are snapshotted on entry and restored on exit (after the capture, which
    executes nothing), so a captured object starts from exactly the state the eager path would have."""

    def __init__(self, module):
        self.bufs = [b for m in module.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
                     for b in (m.running_mean, m.running_var, m.num_batches_tracked) if b is not None]

    def __enter__(self):
        self.saved = [b.detach().clone() for b in self.bufs]
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for b, s_ in zip(self.bufs, self.saved):
            b.copy_(s_)
        return False


class _Capture:
    """what ``capture_scope`` hands to its body: the warm-up stream and the two calls"""

    def __init__(self):
        self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        self._joined = False

    def warm_up(self, fn, n=1):
        """``fn()`` ``n`` times, eagerly, on the side stream"""
        with torch.cuda.stream(self.side):
            for _ in range(n):
                fn()

    def capture(self, fn, on_warmup_stream=False, share_pool=None):
        """a new graph holding one ``fn()``"""
        if not self._joined:
            torch.cuda.current_stream().wait_stream(self.side)
            torch.cuda.synchronize()
            self._joined = True
        graph = torch.cuda.CUDAGraph()
        # No cyclic garbage collection while the stream captures: a pass that starts inside ``fn`` may destroy a dead cycle that
        # holds an earlier captured graph (frame._TrackGraph's closures refer to the object that owns its GraphedInference), and
        # destroying a graph while this thread captures aborted the process (torch.cuda.graph no longer collects on entry).
        # Whatever died waits for the first pass after the capture.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, pool=None if share_pool is None else share_pool.pool(),
                                  stream=self.side if on_warmup_stream else None, capture_error_mode="thread_local"):
                fn()
        finally:
            if gc_was_on:
                gc.enable()
        return graph


@contextlib.contextmanager
def capture_scope(module=None, sampler=None):
    """The choreography of every hipGraph capture of the project, stated once.  ``with capture_scope(module, sampler) as cap:``
    then ``cap.warm_up(fn, n)`` any number of times, then ``cap.capture(fn)`` once per graph (Python may run in between).

    * Timer off.  ``ops.set_timer(None)`` for the whole scope: a KernelTimer records HIP events around every entry point, and
      events cannot be recorded inside a capture.  The previous timer comes back on exit.
    * State rolled back.  The warm-up runs the live ``module`` in train mode on an example batch and advances the ``sampler`` of
      the body's device draws although no step has happened: BatchNorm statistics (``_preserve_bn_stats``) and the sampler's
      state and key (``_keep_sampler_state``) are snapshotted on entry, each only if given, and restored on exit in reverse order
      -- sampler, BatchNorm, timer -- whether or not the body raised.
    * Warm-up on a side stream.  A body has to run eagerly before it is captured (lazy initialisation, the libraries'
      workspaces and autograd's accumulators do work a capture cannot hold), and it runs on a fresh stream that waits for the
      current one, not on the default stream, whose implicit synchronisation a capture forbids.  The streams are joined and the
      device synchronised once, after the last warm-up work and before the first capture.
    * ``thread_local`` error mode.  Other threads of the process (RCCL's watchdog polling events, the autograd engine's workers)
      may call into HIP while this thread captures: only this thread's calls are checked against the capture.
    * ``capture(on_warmup_stream=True)``.  Autograd binds each parameter's gradient accumulator to the stream of its first use,
      and an accumulator bound to another stream than the capture stream is executed OUTSIDE the capture (the replayed graph
      then reads freed memory).  A body whose backward accumulates into the ``.grad`` of parameters that saw no backward before
      the warm-up is therefore captured on the stream its warm-up ran on; every other body on ``torch.cuda.graph``'s own.
    * ``capture(share_pool=graph)``: an earlier graph of the scope whose memory pool the new one allocates from (tensors made
      inside the first capture stay valid inputs of the second)."""
    prev_timer = ops.set_timer(None)
    try:
        with _preserve_bn_stats(module) if module is not None else contextlib.nullcontext(), _keep_sampler_state(sampler):
            yield _Capture()
    finally:
        ops.set_timer(prev_timer)


def _copy_in(pairs):
    """new data into static buffers: ``(dst, src)`` pairs, a ``src`` of None leaves its buffer as it is"""
    for dst, src in pairs:
        if src is not None:
            dst.copy_(src, non_blocking=True)


def _pack_grads(params, grads, out):
    """the gradients as ONE flat buffer (one captured multi-tensor copy), zeros where a parameter has none"""
    torch.cat([(g if g is not None else torch.zeros_like(p)).reshape(-1) for p, g in zip(params, grads)], out=out)


class GraphedStep:
    """step = zero_grad; (_, _, feat) = face_recon(centred, obj); feat.backward(dfeat)   as one hipGraph.

    ``centred`` (B,N,3), ``obj`` (B,1), ``dfeat`` (B,N,1286) are static device buffers owned by this object
    (``load_inputs`` copies new data in); parameter ``.grad`` tensors live in the graph's memory pool
    and are overwritten by every replay; ``feat`` is the static output."""

    def __init__(self, face_recon, centred, obj, dfeat, warmup=3, flat_grads=False, split=False):
        """flat_grads=True additionally packs every parameter gradient into ONE contiguous buffer
        (``self.flat_grad``, one captured multi-tensor copy per step) so a data-parallel caller can
        all-reduce the step's gradients with a single RCCL collective right after the replay.

        split=True (implies flat_grads) captures the step as TWO graphs cut at ``face_recon.backward_cut``:
        ``run_first()`` = zero_grad, forward and the backward of everything above the cut (conv_3, conv_4, bn3:
        78 % of the gradient bytes, ready after the cheap coarse levels) packed into ``flat_late``; ``run_second()`` =
        the backward of the fine levels packed into ``flat_early``.  The caller starts the all-reduce of ``flat_late``
        between the two, so that exchange overlaps the N=1028 layers' backward."""
        self.net = face_recon
        self.centred, self.obj, self.dfeat = centred, obj, dfeat
        B, N, _ = centred.shape
        self.n_points = N
        dev = centred.device
        self.pool_idx = pool_index_buffers(face_recon, N, dev)
        self.params = [p for p in face_recon.parameters() if p.requires_grad]
        self.feat = None
        self.flat_grad = self.flat_late = self.flat_early = None
        self.split = bool(split)
        face_recon.keep_backward_cut = False           # (a split capture of the same network sets it; this object's form decides)
        if flat_grads or split:
            self.flat_grad = torch.zeros(sum(p.numel() for p in self.params), dtype=torch.float32, device=dev)
        self._upload_pool_indices()
        with capture_scope(face_recon) as cap:
            if split:
                cap.warm_up(self._find_late_params)
                cap.warm_up(lambda: (self._body_first(), self._body_second()), warmup)
                self.graph = cap.capture(self._body_first)
                self.graph2 = cap.capture(self._body_second, share_pool=self.graph)
            else:
                cap.warm_up(self._body, warmup)
                self.graph = cap.capture(self._body)

    def _forward(self, zero_grads=True):
        if zero_grads:
            for p in self.params:
                p.grad = None
        with pool_feed(self.pool_idx):
            return self.net(self.centred, self.obj)[2]

    def _body(self):
        feat = self._forward()
        with ops.StepFolds():                           # every p.grad is None: the backward's folds go out in one launch
            feat.backward(self.dfeat)
        self.feat = feat.detach()                       # (keeping the autograd graph alive would pin its accumulators' streams)
        if self.flat_grad is not None:
            _pack_grads(self.params, [p.grad for p in self.params], self.flat_grad)

    # ---- the step cut in two (split=True) -------------------------------------------------------------------------
    def _find_late_params(self):
        """late = the parameters the cut tensors do not depend on (their gradients are complete after the first part).
        ``flat_grad`` is laid out [late | early] so each part is one contiguous all-reduce."""
        self.net.keep_backward_cut = True
        feat = self._forward(zero_grads=False)
        cut = list(self.net.backward_cut)
        self.net.backward_cut = None
        below = torch.autograd.grad(cut, self.params, [torch.zeros_like(c) for c in cut], allow_unused=True)
        self.late = [p for p, g in zip(self.params, below) if g is None]
        self.early = [p for p, g in zip(self.params, below) if g is not None]
        del feat, below
        n_late = sum(p.numel() for p in self.late)
        self.flat_late, self.flat_early = self.flat_grad[:n_late], self.flat_grad[n_late:]
        self.params = self.late + self.early           # grad_views() follows the flat layout

    def _body_first(self):
        feat = self._forward()
        self.feat = feat.detach()
        cut = list(self.net.backward_cut)
        self.net.backward_cut = None
        with ops.StepFolds():
            grads = torch.autograd.grad(feat, cut + self.late, self.dfeat, allow_unused=True)
        self._cut, self._cut_grads = cut, list(grads[:len(cut)])
        _pack_grads(self.late, grads[len(cut):], self.flat_late)

    def _body_second(self):
        with ops.StepFolds():
            torch.autograd.backward(self._cut, self._cut_grads, inputs=self.early)
        _pack_grads(self.early, [p.grad for p in self.early], self.flat_early)
        self._cut = self._cut_grads = None

    def _upload_pool_indices(self):
        upload_pool_indices(self.pool_idx, self.n_points)

    def load_inputs(self, centred=None, obj=None, dfeat=None):
        _copy_in(((self.centred, centred), (self.obj, obj), (self.dfeat, dfeat)))

    def run(self):
        """one step: draw + upload the pool indices (host RNG, reference order), replay the graph."""
        self.run_first()
        if self.split:
            self.run_second()
        return self.feat

    def run_first(self):
        """split=True: pool indices, forward, backward above the cut -> ``flat_late`` is final"""
        self._upload_pool_indices()
        self.graph.replay()
        return self.feat

    def run_second(self):
        """split=True: the rest of the backward -> ``flat_early`` is final"""
        self.graph2.replay()

    def grad_views(self):
        """per-parameter views into flat_grad (after an all-reduce these ARE the averaged gradients)"""
        out, off = [], 0
        for p in self.params:
            out.append(self.flat_grad[off:off + p.numel()].view_as(p))
            off += p.numel()
        return out


def check_accumulate(who, accumulate):
    """the ``accumulate=`` argument of the graphed training steps: an int >= 1, and 1 with more than one rank (each rank's gate
    would decide on its own loss, and the exchange of an accumulated gradient is not built).  Touches no device."""
    if isinstance(accumulate, bool) or int(accumulate) != accumulate or int(accumulate) < 1:
        raise ValueError(f"{who}: accumulate expects an integer >= 1, got {accumulate!r}")
    if int(accumulate) > 1:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError(f"{who}: accumulate > 1 is not offered with more than one rank")
    return int(accumulate)


class GraphedTrainStep:
    """One full training step of engine/train.py:76-104 with the device work replayed as a hipGraph:

        zero_grad -> HSPose.forward(do_loss=True) (augmentation, network, 19 losses) -> sum -> backward -> squared
        gradient norm                                              [captured once, replayed]
        optimizer.step() (clip coefficient applied inside) ; scheduler.step()      [one launch + host scalars; with
                                                                    apply='graph' gated on the device, inside the replay]

    Host work before each replay, in the reference's order on the CPU default generator: the jitter factors of
    ``defor_3D_pc`` (``torch.rand(PC.shape) * aug_pc_r``) and the two Pool_layer ``randperm`` draws; the augmentation's
    ``torch.rand(..., device=...)`` draws are made inside the graph by the device generator.  ``batch`` is a dict of
    static device tensors with HSPose.forward's keyword names (``load_batch`` copies new data in); gradients land in
    the fused optimizer's flat buffer.  Eagerly the step is CPU-bound (~2500 tiny launches in the losses alone).

    Runtime note.  In round 1 the step still held ATen multi-block reductions (bias-gradient column sums over 16448 rows,
    ``max`` over the points, the ~2 200 small kernels of the losses) and two of them replayed with wrong results under ROCm
    7.2's default AQL-packet capture of graph kernel nodes, so the constructor demanded ``DEBUG_CLR_GRAPH_PACKET_CAPTURE=0``.
    With the heads on ``ops.linear_rows`` / ``ops.points_max`` and the losses in libhsp's five kernels the captured step
    replays equal to the eager step under the DEFAULT runtime (tests/test_gpu_train_graph.py, B=4 N=256 and B=16 N=1028:
    every loss term, gradient and updated parameter), and the flag is no longer needed.  Rounds 2-5 measured ``run()`` at
    30 ms per step at B=16 N=1028 and blamed the runtime's execution of the graph; round 6 found the replay itself takes the
    kernels' 8.0 ms and the rest was HOST time in ``_host_draws``: the jitter draw was scaled by a 49 k-element CPU multiply
    that woke an over-subscribed OpenMP pool (8 ms) and uploaded from pageable memory (a wait for the previous replay).  With
    the draw scaled in serial pieces into the pinned ring, ``run()`` is 8.2 ms -- replay + 0.15 ms -- and this is the form
    ``bench.py`` reports for unit U3.

    Build it BEFORE the network's first eager backward: the gradient accumulators have to be bound to the capture stream, which
    is the stream of the warm-up here (``capture_scope``: ``on_warmup_stream``) and cannot be once an eager backward has run.

    ``prologue``: a callable issued at the head of the captured body, on the capture stream, that returns a dict; its entries
    replace the same-named entries of ``batch`` for that body -- the step in front of the network captured with it
    (train.FrameTrainStep: the training loader's front end and the choice of the kept items).  It reads static buffers of its
    owner's and must be issuable both eagerly (the warm-up) and under capture; ``batch`` then gives the shapes and the static
    buffers of the other keys only, and ``load_batch`` has no effect on the replaced ones.  None: the body is the batch's.

    ``draws``: who makes the step's draws, resolved when the object is built (``pc_sample.resolve_draws``: None follows
    ``FLAGS.step_draws``).  Under a device sampler the captured body begins with the keyed draw of both Pool_layers' rows into the
    static index buffers and its augmentation is ``hsp_pose_augment_keyed``; there is no host work before a replay and no
    generator is touched: THE OWNER CALLS ``draws.advance()`` BEFORE EACH ``replay()`` / ``run()`` (the 16-byte key upload), and
    equal sampler states replay equal steps.  Building the object leaves the sampler's state as it found it.

    ``apply``: who applies the step.  'host' (default) is all of the above.  'graph': the body goes on, inside the capture, with
    ``hsp_step_gate`` on the total loss (and on ``gate_info``, ``hsp_batch_select``'s info, when given) and the gated Ranger launch
    (``solver.DeviceClock`` over ``Ranger.device_clock(scheduler, horizon)``).  ``replay()`` is then the
    step, ``run()`` is ``replay()``, ``apply()`` raises, and ``run(check_nan=True)`` reads the device's decision back after the
    replay -- it reports the skip, it no longer makes it.  Under device draws a ``run()`` is the owner's ``draws.advance()`` plus one
    graph launch and nothing else.  ``horizon``: the number of applied steps tabulated (default: the rest of the scheduler's
    ``total_iters``); a step past it is refused on the device (``exhausted``), build a new object to go on.
      * The warm-up runs execute both new kernels UNARMED: parameters, moments, slow weights and counters stay as they were;
        the constructor arms the gate once, after the capture.
      * On a skipped step the BatchNorm running statistics HAVE moved: the forward ran before the loss was known.  The
        reference behaves the same (its forward precedes its NaN test, engine/train.py:76-95).
      * ``scheduler.step()`` and ``optimizer.step()`` are never called in this form.  THE SCHEDULER OBJECT, ``state[p]['step']``
        AND THE GROUPS' ``lr`` ARE CURRENT ONLY AFTER ``optimizer.sync_clock()`` (one small copy and a wait; ``optimizer.state_dict()``
        and ``TrainDriver.checkpoint()`` call it), which also returns the counters: applied, replays, skipped_nan,
        skipped_no_item, exhausted.
      * No data parallelism in this form.

    ``accumulate`` (default 1: nothing below applies, no code path changes): gradient accumulation as the reference has it,
    quirks included (engine/train.py:99-114; tests/_accum_ref.py states the rules in plain Python).  THE
    ARGUMENT IS NOT TAKEN FROM ``FLAGS.accumulate``: pass ``TrainDriver.accumulate``.  A counter ``micro`` plays the reference's
    ``global_step``: it starts at ``global_step`` and advances on every replay, skipped ones included.  A replay whose loss is NaN
    (or, with ``gate_info``, whose batch has no good item) is SKIPPED: its gradient stays out of the accumulator and nothing is
    applied.  Otherwise the slot is TAKEN: the fresh gradient -- the body moves it into the optimizer's second flat buffer
    (``_FlatGroup.flat_f``) and runs no ``clip_grad_norm_`` of its own -- is added to the accumulator (``flat_g``) by
    ``hsp_grad_accumulate``, which also leaves the accumulator's squared norm beside it; the step (optimizer, scheduler, and
    what stands for ``zero_grad``) is applied exactly when ``micro % accumulate == 0``, with the clip coefficient of the
    ACCUMULATED gradient; on any other taken slot that coefficient is the reference's in-place clip, deferred into the next take.
    Slot 0 steps on its own gradient alone, and a skipped stepping slot lets the accumulator grow until the next
    ``micro % accumulate == 0``.  No memset follows a step: while nothing is pending the accumulator's contents mean nothing
    (``optimizer.accumulated_grads()`` gives what ``p.grad`` would hold in the eager driver).
      * ``apply='graph'``: gate (``hsp_step_gate_accum``), gated accumulate and gated Ranger launch are inside the capture;
        ``run()`` stays the owner's ``advance()`` plus one graph launch, ``run(check_nan=True)`` returns whether the slot was
        TAKEN, and ``optimizer.sync_clock()`` reports ``micro`` and ``pending`` with the other counters.
      * ``apply='host'``: ``replay()`` ends at the fresh buffer; ``apply()`` issues the accumulate and, on a stepping slot,
        ``optimizer.step()`` and ``scheduler.step()``; ``run(check_nan=True)`` skips ``apply()`` on a NaN loss and still advances
        ``micro`` (``skip()``); the host keeps ``micro`` and ``pending`` (``optimizer._accum``).
      * More than one rank is refused in both forms; ``TrainDriver.checkpoint()`` carries the accumulator while one is pending."""

    def __init__(self, network, optimizer, batch, scheduler=None, max_norm=5, warmup=3, prologue=None, draws=None,
                 apply="host", horizon=None, gate_info=None, accumulate=1, global_step=0):
        self.accumulate = check_accumulate("GraphedTrainStep", accumulate)      # (before anything touches the device)
        if apply not in ("host", "graph"):
            raise ValueError(f"GraphedTrainStep: apply expects 'host' or 'graph', got {apply!r}")
        self.net, self.opt, self.sched, self.max_norm = network, optimizer, scheduler, max_norm
        self.batch = batch
        self._prologue = prologue
        # apply='graph': tables and the UNARMED control block go up here, before the warm-up (an upload cannot be captured)
        self.clock = (optimizer.device_clock(scheduler, horizon, info=gate_info, accumulate=self.accumulate, global_step=global_step)
                      if apply == "graph" else None)
        # accumulate > 1: flat_g becomes the accumulator, the fresh gradient gets a flat buffer of its own (made here, once)
        self.accum = optimizer.accumulation(self.accumulate, global_step, max_norm, clock=self.clock) if self.accumulate > 1 else None
        if self.accum is None:
            optimizer._accum = None                          # (an earlier accumulating object on this optimizer no longer speaks for it)
        PC = batch["PC"]
        B, N, _ = PC.shape
        self.n_points = N
        dev = PC.device
        self.draws = pc_sample.resolve_draws(draws, dev)
        self.noise = torch.zeros_like(PC) if self.draws is None else None
        self.pool_idx = pool_index_buffers(network, N, dev)
        self.loss_dict, self.total = None, None
        self._host_draws()
        with capture_scope(network, self.draws) as cap:
            cap.warm_up(self._body, warmup)
            # capture ON THE WARM-UP STREAM: the parameters' gradient accumulators were bound to it by the warm-up backward
            self.graph = cap.capture(self._body, on_warmup_stream=True)
        if self.clock is not None:
            self.clock.arm()                                 # once, after the capture: from here on a replay is a step

    def _host_draws(self):
        if self.draws is not None:                           # device draws: everything is drawn inside the replay
            return
        if FLAGS.train:
            # (through the pinned ring, like the pool indices: a copy from pageable memory waits for the previous replay, and the
            # host then cannot queue step i + 1 under step i -- 8 ms of replay + the graph launch's own host time per step, measured
            # 21-41 ms where the replay alone takes 8.1)
            # The scaling runs in pieces below ATen's parallel grain (32768 elements): a 49 k-element multiply wakes the whole
            # OpenMP pool, and with more threads than the container has cores (128 vs a 16-CPU quota on the GPU box) that one
            # multiply cost 8 ms of host time per step.
            r = FLAGS.aug_pc_r

            def fill(pinned):
                src, dst = torch.rand(self.noise.shape).view(-1), pinned.view(-1)
                for o in range(0, src.numel(), 16384):
                    torch.mul(src[o:o + 16384], r, out=dst[o:o + 16384])
            staging.upload(fill, self.noise.shape, torch.float32, self.noise.device, out=self.noise)
        upload_pool_indices(self.pool_idx, self.n_points)

    def _body(self):
        # Gradients are created INSIDE the capture (grad = None first) and then moved into the optimizer's flat buffer
        # with one multi-tensor copy: accumulating straight into the pre-existing flat views makes autograd synchronise
        # the capture stream with the stream those views were made on, and the replayed graph then waits forever.
        with pc_sample.draw_scope(self.draws or "host", self.batch["PC"].device) as scope:
            draw_pool_rows(scope, self.pool_idx, self.n_points)
            batch = self.batch if self._prologue is None else {**self.batch, **self._prologue()}
            params, views = self._params_and_views()
            for p in params:
                p.grad = None
            noise = augment.jitter_noise_feed(self.noise) if scope is None else contextlib.nullcontext()
            with pool_feed(self.pool_idx), noise:
                od, ld = self.net(do_loss=True, **batch)
        self.output_dict = {k: v.detach() for k, v in od.items() if isinstance(v, torch.Tensor)}    # static: every replay rewrites them
        total = self.net.total_loss(ld)                     # (the sum over the four sub-dictionaries, engine/train.py:84-90)
        with ops.StepFolds():
            total.backward()
        torch._foreach_copy_(views, [p.grad if p.grad is not None else torch.zeros_like(p) for p in params])
        if self.accum is not None:
            self._body_accumulate(ld, total)
            return
        for p, v in zip(params, views):
            p.grad = v
        self.opt.clip_grad_norm_(self.max_norm)             # device scalar; consumed by the step() outside the graph
        self._gnorm_sq, self._max_norm = self.opt._gnorm_sq, self.opt._max_norm
        self.loss_dict, self.total = ld, total
        if self.clock is not None:                          # apply='graph': the device decides on the loss, then steps or does not
            self.clock.gate(total.detach())
            self.clock.step()

    def _body_accumulate(self, ld, total):
        """accumulate > 1: the fresh gradient is in ``flat_f``; ``.grad`` names the accumulator's views.  No norm of the fresh
        gradient: the clip acts on the accumulated one (``hsp_grad_accumulate``)."""
        fg = self.opt._flat[0]
        for p, o in zip(fg.params, fg.offsets):
            p.grad = fg.view(fg.flat_g, p, o)
        self.loss_dict, self.total = ld, total
        if self.clock is not None:                          # apply='graph': gate -> accumulate (gated) -> gated Ranger launch
            self.clock.gate(total.detach())
            self.accum.take()
            self.opt._gnorm_sq, self.opt._max_norm = self.accum.norm_sq, self.accum.max_norm
            self.clock.step()

    def _params_and_views(self):
        params, views = [], []
        for fg in self.opt._flat:
            flat = fg.flat_g if self.accum is None else fg.flat_f
            for p, o in zip(fg.params, fg.offsets):
                params.append(p)
                views.append(fg.view(flat, p, o))
        return params, views

    def load_batch(self, batch):
        _copy_in((self.batch[k], v) for k, v in batch.items())

    def replay(self):
        """the host draws and the replay: losses and gradients of one step, nothing applied yet (device draws: the replay
        alone, under the key of the owner's last ``draws.advance()``)"""
        self._host_draws()
        self.graph.replay()

    def apply(self):
        """the fused optimizer launch (clip coefficient inside) and the scheduler, behind ``replay()``"""
        if self.clock is not None:
            raise RuntimeError("GraphedTrainStep(apply='graph'): the step is applied inside the replay; there is nothing to apply()")
        if self.accum is not None:                           # the taken slot of engine/train.py:105-114
            acc = self.accum
            acc.take(first=acc.pending == 0)
            acc.pending += 1
            if acc.micro % acc.accumulate == 0:
                self.opt._gnorm_sq, self.opt._max_norm = acc.norm_sq, acc.max_norm
                self.opt.step()
                if self.sched is not None:
                    self.sched.step()
                acc.pending = 0                              # (zero_grad: the next take starts a fresh accumulator)
            acc.micro += 1
            return
        self.opt._gnorm_sq, self.opt._max_norm = self._gnorm_sq, self._max_norm
        self.opt.step()
        if self.sched is not None:
            self.sched.step()

    def skip(self):
        """``apply='host'``: the owner found this replay's slot skipped (NaN loss, no good item) and will not ``apply()`` it.
        Under accumulation the slot still passes -- ``micro`` advances --; otherwise there is nothing to do."""
        if self.accum is not None and self.clock is None:
            self.accum.micro += 1

    def run(self, check_nan=False):
        """one training step; returns False when ``check_nan`` found a NaN loss (the reference's skip, train.py:91-95).
        ``apply='graph'``: the replay IS the step, and ``check_nan`` only reads the device's decision back (the one wait):
        whether the step was applied or, under accumulation, whether the slot was taken."""
        self.replay()
        if self.clock is not None:
            if not check_nan:
                return True
            return self.clock.applied_last() if self.accum is None else self.clock.taken_last()
        if check_nan and bool(torch.isnan(self.total).any()):
            self.skip()
            return False
        self.apply()
        return True


class GraphedInference:
    """The timed body of the reference's evaluation loop (evaluation/evaluate.py:90-106) as one hipGraph, for a fixed
    number of instances per call:

        output_dict = network(PC, obj_id, mean_shape, sym)         # eval mode: BatchNorm on running statistics
        pred_RT = generate_RT([p_green_R, p_red_R], [f_green_R, f_red_R], Pred_T, mode='vec', sym)
        pred_s = Pred_s + mean_shape

    ``PC`` (n,N,3), ``obj_id`` (n,) or (n,1), ``mean_shape`` (n,3), ``sym`` (n,4) are static device buffers
    (``load`` copies new data in); ``run()`` draws the two Pool_layer permutations on the host generator like the
    reference's forward does, replays, and returns the static ``(pred_RT (n,4,4), pred_s (n,3), output_dict)``.
    A detector producing a varying instance count keeps one object per count (a capture is a few ms).

    ``prologue``: a callable issued at the head of the captured body, on the capture stream, whose result (n,N,3) IS the
    cloud the network reads -- the step in front of the network captured with it (frame.FramePipeline(one_graph=True): the
    frame front end).  It reads static buffers of its owner's; ``PC`` then only gives the shape and ``load(PC=...)`` has no
    effect.

    ``epilogue``: a callable issued at the tail of the captured body, given this object once ``pred_RT`` / ``pred_s`` are
    made -- the step behind the poses captured with them (frame.FrameTracker: the tracked state takes the new poses).  The
    warm-up runs it too: an owner whose epilogue writes state puts that state back after the construction.

    ``draws``: as ``GraphedTrainStep``'s -- under a device sampler the body begins with the keyed draw of the Pool_layers' rows,
    ``run()`` is the replay alone, and the owner calls ``draws.advance()`` before it."""

    def __init__(self, network, PC, obj_id, mean_shape, sym, warmup=2, prologue=None, draws=None, epilogue=None):
        from .geom_utils import generate_RT
        self.net, self._generate_RT = network, generate_RT
        self.PC, self.obj_id, self.mean_shape, self.sym = PC, obj_id, mean_shape, sym
        self._prologue, self._epilogue = prologue, epilogue
        n, N, _ = PC.shape
        self.n_points = N
        dev = PC.device
        self.pool_idx = pool_index_buffers(network, N, dev)
        if network.training:
            raise RuntimeError("GraphedInference: put the network in eval() mode first")
        self.draws = pc_sample.resolve_draws(draws, dev)
        self._draw()
        with capture_scope(sampler=self.draws) as cap:       # (eval mode: no BatchNorm statistics move)
            cap.warm_up(self._body, warmup)
            self.graph = cap.capture(self._body)

    def _draw(self):
        if self.draws is None:                               # (device draws: the rows are drawn inside the replay)
            upload_pool_indices(self.pool_idx, self.n_points)

    @torch.no_grad()
    def _body(self):
        with pc_sample.draw_scope(self.draws or "host", self.obj_id.device) as scope:
            draw_pool_rows(scope, self.pool_idx, self.n_points)
            if self._prologue is not None:
                self.PC = self._prologue()
            with pool_feed(self.pool_idx):
                out = self.net(PC=self.PC, obj_id=self.obj_id, mean_shape=self.mean_shape, sym=self.sym)
        self.pred_RT = self._generate_RT([out['p_green_R'], out['p_red_R']], [out['f_green_R'], out['f_red_R']],
                                         out['Pred_T'], mode='vec', sym=self.sym)
        self.pred_s = out['Pred_s'] + self.mean_shape
        self.output_dict = out
        if self._epilogue is not None:
            self._epilogue(self)

    def load(self, PC=None, obj_id=None, mean_shape=None, sym=None):
        _copy_in(((self.PC, PC), (self.obj_id, obj_id), (self.mean_shape, mean_shape), (self.sym, sym)))

    def run(self):
        self._draw()
        self.graph.replay()
        return self.pred_RT, self.pred_s, self.output_dict


class _GraphedNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner, anchor):
        ctx.runner = runner
        runner.graph_fwd.replay()
        outs = tuple(o.detach() for o in runner.outs)
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        r = ctx.runner
        for buf, g in zip(r.gouts, gouts):
            if g is None:
                buf.zero_()
            else:
                buf.copy_(g)
        r.graph_bwd.replay()
        have = [(p, g) for p, g in zip(r.params, r.pgrads) if g is not None]
        acc = [(p.grad, g) for p, g in have if p.grad is not None]
        if acc:
            torch._foreach_add_([a for a, _ in acc], [g for _, g in acc])
        for p, g in have:
            if p.grad is None:
                p.grad = g.clone()
        return None, None


class GraphedNetwork:
    """``posenet(PC, obj_id)`` of a training step as two hipGraphs behind ONE autograd node: the forward graph produces
    the ten network outputs in static buffers, the backward graph takes their gradients from static buffers and leaves
    the parameter gradients in static buffers, which the node adds into ``p.grad`` with one multi-tensor add.  Losses,
    augmentation and the optimizer stay eager (they are not part of the captured region), so this is the part of
    ``engine/train.py``'s step that is pure kernels + library GEMMs: ~400 launches and their autograd bookkeeping become
    two replays.  The network's Conv1d(k=1) layers go through ``ops.linear_rows`` (bias gradient by the column-sum
    kernels), BatchNorm through ``ops.bn_relu`` and the max over points through ``ops.points_max``, so the captured
    graphs contain no ATen multi-block reduction (see GraphedTrainStep for why that matters on ROCm 7.2).

    ``runner = GraphedNetwork(net.posenet, PC, obj_id)`` (example inputs of the step's shape, B and N fixed);
    ``outs = runner(PC, obj_id)`` inside the usual step, ``loss.backward()`` as usual.  The returned tensors ALIAS the
    graph's static output buffers: the next call overwrites them -- ``clone()`` anything kept across steps.  Constructing
    the object leaves the BatchNorm running statistics untouched (warm-up runs are rolled back).  The Pool_layer permutations are
    drawn on the host generator before every replay, dropout uses the device generator inside the graph."""

    def __init__(self, posenet, PC, obj_id, warmup=3):
        self.net = posenet
        self.PC = PC.detach().clone()
        self.obj_id = obj_id.detach().clone()
        B, N, _ = PC.shape
        self.n_points = N
        dev = PC.device
        self.pool_idx = pool_index_buffers(posenet, N, dev)
        self.params = [p for p in posenet.parameters() if p.requires_grad]
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)
        upload_pool_indices(self.pool_idx, N)
        with capture_scope(posenet) as cap:
            cap.warm_up(self._warm, warmup)
            self.graph_fwd = cap.capture(self._capture_forward)
            self.gouts = [torch.zeros_like(o) for o in self.outs]
            self.graph_bwd = cap.capture(self._capture_backward, share_pool=self.graph_fwd)

    def _forward(self):
        with pool_feed(self.pool_idx):
            return self.net(self.PC, self.obj_id)

    def _warm(self):
        outs = self._forward()
        live = [o for o in outs if o is not None and o.requires_grad]
        torch.autograd.grad(live, self.params, [torch.zeros_like(o) for o in live], allow_unused=True)

    def _capture_forward(self):
        outs = self._forward()
        self.none_mask = [o is None for o in outs]
        self.outs = [o for o in outs if o is not None]

    def _capture_backward(self):
        with ops.StepFolds(bare_wgrad=True):            # (before the .contiguous() copies below read the gradients)
            self.pgrads = list(torch.autograd.grad(self.outs, self.params, self.gouts, allow_unused=True))
        # contiguous static gradients (copies inside the graph where autograd hands back a transposed view): the
        # multi-tensor add of the node then takes its fused path instead of one small kernel per parameter
        self.pgrads = [g if g is None or g.is_contiguous() else g.contiguous() for g in self.pgrads]

    def __call__(self, PC, obj_id):
        if PC.shape != self.PC.shape:
            raise RuntimeError(f"GraphedNetwork was captured for {tuple(self.PC.shape)}, got {tuple(PC.shape)}")
        self.PC.copy_(PC)
        self.obj_id.copy_(obj_id.reshape(self.obj_id.shape))
        upload_pool_indices(self.pool_idx, self.n_points)
        live = iter(_GraphedNetFn.apply(self, self._anchor))
        return tuple(None if isnone else next(live) for isnone in self.none_mask)
