"""Train-step driver semantics of the reference's ``engine/train.py:72-130``, around the fused
optimizer of ``hs_pose_amd.solver``:

  total_loss NaN -> the iteration is skipped (counters advance, nothing else happens)       train.py:91-95
  backward; clip_grad_norm_(network.parameters(), 5) after EVERY backward -- on iterations that only accumulate the
  coefficient is applied to the accumulated gradients in place, like the reference's in-place clip; on stepping
  iterations it is folded into the fused optimizer step                                      train.py:98-99,103-104
  optimizer.step(); scheduler.step(); optimizer.zero_grad() when global_step % accumulate == 0   train.py:97-102
  checkpoint = {'seed','epoch','posenet_state_dict','scheduler','optimizer'}                 train.py:115-123

``TrainDriver.step(total_loss)`` is the body of that loop for one batch.  With ``check_nan=False`` the NaN test
(the loop's only host synchronisation besides logging) is skipped.

``FrameTrainStep`` is that step started from raw frames: the training loader's front end (``pc_sample.train_batch_to_pcl``), the
choice of the kept items (``pc_sample.train_batch_select``) and ``graph.GraphedTrainStep``'s body as ONE replay.
``RenderedTrainStep`` is ``FrameTrainStep`` with the frames themselves drawn and rendered at the head of that replay
(``render.SceneSource``): a synthetic training step as a pure function of the sampler's {seed, call} and the mesh set.
"""
import math

import numpy as np
import torch
import torch.distributed as dist

from . import ops, pc_sample
from .config import FLAGS
from .graph import GraphedTrainStep, check_accumulate
from .parallel import mean_flat_gradients
from .solver import build_lr_rate, build_optimizer


class TrainDriver:
    def __init__(self, network, optimizer=None, scheduler=None, total_iters=None, accumulate=None, max_norm=5,
                 check_nan=True, global_step=0, data_parallel=None, draws=None):
        """draws: the ``pc_sample.DeviceSampler`` that keys the run's device draws (``FLAGS.step_draws = 'device'``), if any: its
        state then travels in the checkpoint, so a resumed run draws what the uninterrupted one would have drawn.

        data_parallel (default: whenever torch.distributed is initialised with more than one rank): after every
        backward the gradients -- already in the optimizer's flat buffers -- are averaged over the ranks with one RCCL
        all-reduce per parameter group, before clipping (the reference trains on a single device, train.py:23)."""
        self.network = network
        if data_parallel is None:
            data_parallel = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.data_parallel = bool(data_parallel)
        self.optimizer = optimizer if optimizer is not None else build_optimizer(network.build_params(training_stage_freeze=[]))
        if getattr(network, "feature_dtype", torch.float32) == torch.bfloat16:
            # the fused optimizer re-seats the parameters in its flat buffers: fresh bf16 working copies of the new storage
            network.set_feature_dtype(torch.bfloat16)
        if scheduler is None:
            if total_iters is None:
                acc = int(accumulate if accumulate is not None else getattr(FLAGS, "accumulate", 1))
                total_iters = int(getattr(FLAGS, "train_steps", 1500)) * int(getattr(FLAGS, "total_epoch", 150)) // acc   # train.py:51
            scheduler = build_lr_rate(self.optimizer, total_iters=total_iters)
        self.scheduler = scheduler
        self.accumulate = int(accumulate if accumulate is not None else getattr(FLAGS, "accumulate", 1))
        self.max_norm = max_norm
        self.check_nan = check_nan
        self.global_step = int(global_step)
        self.skipped = 0
        if draws is not None and not isinstance(draws, pc_sample.DeviceSampler):
            raise ValueError(f"TrainDriver: draws expects a pc_sample.DeviceSampler or None, got {draws!r}")
        self.draws = draws

    def step(self, total_loss):
        """one batch of engine/train.py's loop; returns False when the batch was skipped for a NaN loss."""
        if self.check_nan and math.isnan(float(total_loss.detach())):
            print('Found nan in total loss')
            self.global_step += 1
            self.skipped += 1
            return False
        total_loss.backward()
        if self.data_parallel:                                 # one process per GPU: gradient mean over the ranks
            self.optimizer.sync_grads()                        # (a backward may have re-created .grad outside the flat buffer)
            mean_flat_gradients([fg.flat_g for fg in self.optimizer._flat])
        self.optimizer.clip_grad_norm_(self.max_norm)
        if self.global_step % self.accumulate == 0:
            self.optimizer.step()
            self.scheduler.step()
            self.optimizer.zero_grad()
        else:
            self.optimizer.scale_grads_by_clip_()              # accumulate-only iteration: clip in place (train.py:103-104)
        self.global_step += 1
        return True

    def checkpoint(self, seed, epoch):
        """the dict engine/train.py:115-123 passes to torch.save (same keys, same sub-layouts); with a device sampler also
        'draws': its (seed, call) state.  With a device clock on the optimizer (``apply='graph'``) the host's mirror of the step
        count and the schedule is brought up to date first (``Ranger.sync_clock``: one small copy, a wait).  With gradient
        accumulation attached to the optimizer (``GraphedTrainStep(accumulate=...)``) and micro-batches pending, also 'accum':
        {'micro', 'pending', 'grad' (the accumulator), 'norm_sq'} -- the reference saves no gradients; this is for the
        bit-reproducible resume.  With nothing pending the keys are the reference's."""
        if getattr(self.optimizer, "_clock", None) is not None:
            self.optimizer.sync_clock()                        # before the scheduler is read below
        ckpt = {
            'seed': seed,
            'epoch': epoch,
            'posenet_state_dict': self.network.state_dict(),
            'scheduler': self.scheduler.state_dict(),
            'optimizer': self.optimizer.state_dict(),
        }
        if self.draws is not None:
            ckpt['draws'] = tuple(self.draws.get_state())
        accum = getattr(self.optimizer, "_accum", None)
        state = accum.state() if accum is not None else None   # (None while nothing is pending: the keys stay as they were)
        if state is not None:
            ckpt['accum'] = state
        return ckpt

    def load_checkpoint(self, ckpt):
        """resume (engine/train.py:53-59: model weights, optimizer and scheduler state when present); returns the epoch
        to START from, i.e. the checkpoint's epoch + 1 like the reference's ``s_epoch``."""
        self.network.load_state_dict(ckpt['posenet_state_dict'])
        if 'optimizer' in ckpt:
            self.optimizer.load_state_dict(ckpt['optimizer'])
        if 'scheduler' in ckpt:
            self.scheduler.load_state_dict(ckpt['scheduler'])
        if getattr(self.optimizer, "_clock", None) is not None:
            self.optimizer._clock.rebuild()                    # tables from the loaded step count AND the loaded epoch
        if self.draws is not None and 'draws' in ckpt:
            self.draws.set_state(ckpt['draws'])
        accum = getattr(self.optimizer, "_accum", None)
        if accum is not None:                                  # after the clock's rebuild, which leaves micro / pending alone
            accum.load_state(ckpt.get('accum'))
        return ckpt.get('epoch', -1) + 1


class FrameTrainStep:
    """One training step from raw frames: a batch of ``M`` items with spares goes in, the first ``keep`` good ones are picked
    on the device, and augmentation, network, the 19 losses, backward and the squared gradient norm follow in the same
    hipGraph; ``run()`` is one replay followed by the fused optimizer launch -- or, with ``apply='graph'``, one replay that
    holds the optimizer launch as well.

    ``frames``: depth (M,H,W) uint16 or fp32 mm and labels (M,H,W) uint8 on the device, inst_ids (M,), bboxes_xyxy (M,4) on the
    host, K (3,3) or (M,3,3).  ``items``: the per-item device tensors of ``HSPose.forward`` with M rows (obj_id, gt_R, gt_t,
    gt_s, mean_shape, sym, aug_bb, aug_rt_t, aug_rt_r, model_point, nocs_scale).  M >= keep: the loader sends keep items plus
    spares.  Both are copied into static buffers; ``load(frames=..., items=...)`` copies the next M items in (device copies and
    the pinned ring: nothing waits).  n_pts, out_size, min_pts and mask_pro are ``train_batch_to_pcl``'s, fixed when the
    object is built; the sampler (None: the module's) is ``train_batch_to_pcl``'s device sampler.

    Host work per ``run()``, in this fixed order: (1) ``pc_sample.dzi_windows(bboxes_xyxy, H, W)`` on numpy's generator -- M
    windows in item order, spares included -- whose transform rows go up through the pinned ring; (2) ``sampler.advance()``;
    (3) ``GraphedTrainStep``'s own draws on the CPU default generator: the jitter noise of keep clouds, then the two
    ``randperm``s.  Then the replay, then the optimizer launch and ``scheduler.step()`` outside the graph.

    A rejected item (``train_batch_to_pcl``'s status) is answered as the reference loader answers it, by moving on to the next
    index: ``sel`` (keep,) int32 names the items the step trained on, ``info`` (2,) int32 = [good items, min(good items, keep)],
    both static device tensors (include/hsp.h: hsp_batch_select); ``batch`` is the selected batch itself, clouds included, and
    ``status`` (M,) the front end's verdict on every item, static too.  With fewer than keep good items the good ones repeat;
    with none the network runs on ``pc_sample.stand_in_cloud`` and the extras of items 0 .. keep-1, never on NaN rows.

    ``run(check=True)`` reads info and the loss's NaN flag after the replay -- one small device->host copy, the cost of
    ``GraphedTrainStep.run(check_nan=True)`` -- and returns False, with neither optimizer step nor scheduler step, when no item
    was good or the loss is NaN (the reference's skip, engine/train.py:91-95).  ``run(check=False)`` never waits: AN
    ALL-REJECTED BATCH THEN TRAINS ONE STEP ON THE STAND-IN CLOUD.  ``info[0] == 0`` says when that happened; the remedy is
    more spares.

    Build it before the network's first eager backward (see ``GraphedTrainStep``).  Building draws like one ``run()`` does on
    numpy's and torch's generators (the warm-up needs windows and noise) and leaves the sampler's state as it found it.

    ``draws``: None (follow ``FLAGS.step_draws`` as it stands when the object is built), 'host' -- all of the above -- or
    'device' / a DeviceSampler: the object's sampler then keys EVERY draw of the step.  ``bboxes_xyxy`` goes to a static int32
    device buffer (data, not a draw), the captured prologue begins with ``hsp_dzi_windows`` ('uniform' DZI only), the body with
    the Pool_layers' keyed rows, the augmentation is ``hsp_pose_augment_keyed``, and ``run()`` is ``sampler.advance()``, the
    replay, the check and the optimizer launch: no generator of the host's is touched, when the object is built or later, and
    equal sampler states give equal steps.

    ``apply='graph'`` (``horizon``: see ``GraphedTrainStep``): the gate on ``info`` and the loss's NaN flag, the schedule and the
    optimizer launch are inside the replay too.  ``run(check=False)`` is then SAFE -- an all-rejected batch or a NaN loss leaves
    parameters and optimizer state untouched and is counted on the device (``skipped_no_item``, ``skipped_nan``) -- and never
    waits; ``run(check=True)`` reads the device's decision back and returns it.  The scheduler object and the optimizer's step
    counts are current only after ``optimizer.sync_clock()``; on a skipped step the BatchNorm statistics have moved.

    ``accumulate``, ``global_step``: ``GraphedTrainStep``'s gradient accumulation, passed on (pass ``TrainDriver.accumulate``; the
    flag is not followed implicitly).  A slot without a good item behaves like a NaN slot in both forms: it passes, nothing enters
    the accumulator, nothing is applied.  With ``run(check=True)`` and ``apply='graph'`` the answer is whether the slot was TAKEN."""

    def __init__(self, network, optimizer, frames, items, keep, scheduler=None, sampler=None, n_pts=None, out_size=None,
                 min_pts=50, mask_pro=None, max_norm=5, warmup=3, draws=None, apply="host", horizon=None, accumulate=1,
                 global_step=0):
        check_accumulate("FrameTrainStep", accumulate)          # (before anything touches the device)
        depth = frames["depth"]
        dev = depth.device
        if depth.dim() != 3 or not 1 <= int(keep) <= depth.shape[0]:
            raise ValueError(f"FrameTrainStep: expects depth (M,H,W) with 1 <= keep <= M, got {tuple(depth.shape)}, keep {keep}")
        self.M, self.H, self.W = depth.shape
        self.keep = int(keep)
        self.n_pts = int(FLAGS.random_points if n_pts is None else n_pts)
        self.out_size = int(FLAGS.img_size if out_size is None else out_size)
        self.sampler = pc_sample.draws_only(pc_sample.resolve_sampler("device" if sampler is None else sampler, dev),
                                             "FrameTrainStep")
        if self.sampler is None:
            raise ValueError("FrameTrainStep: expects a device sampler; there is no host-draw form of the training front end")
        self.draws = self.sampler if pc_sample.resolve_draws(draws, dev) is not None else None
        if self.draws is not None and str(FLAGS.DZI_TYPE).lower() != "uniform":
            raise NotImplementedError(f"FrameTrainStep: the device draws build DZI_TYPE 'uniform' only, got {FLAGS.DZI_TYPE!r}")
        self.bboxes_d = torch.zeros(self.M, 4, dtype=torch.int32, device=dev)
        self.depth = depth.detach().clone()
        self.labels = frames["labels"].detach().clone()
        self.inst_ids = torch.empty(self.M, dtype=torch.int32, device=dev)
        self.xf = torch.empty(self.M, 3, dtype=torch.float64, device=dev)
        self.K = torch.empty(self._K_rows(frames["K"]).shape, dtype=torch.float64, device=dev)
        self.items = {k: v.detach().clone() for k, v in items.items()}
        for k, v in self.items.items():
            if not v.is_cuda or v.dim() < 1 or v.shape[0] != self.M:
                raise ValueError(f"FrameTrainStep: items[{k!r}] expects a device tensor with {self.M} rows, got {tuple(v.shape)}")
        self.sel = torch.zeros(self.keep, dtype=torch.int32, device=dev)
        self.info = torch.zeros(2, dtype=torch.int32, device=dev)
        self.status = self.batch = None
        self._load_small(frames)
        pc_sample.stand_in_cloud(self.n_pts, dev)               # (made here: an upload cannot happen inside the capture)

        dzi = (float(FLAGS.DZI_PAD_SCALE), float(FLAGS.DZI_SCALE_RATIO), float(FLAGS.DZI_SHIFT_RATIO))

        def front_end():
            self._scene()
            if self.draws is not None:                          # the windows of this replay, drawn under its key
                ops.dzi_windows_device(self.bboxes_d, self.sampler.key, self.H, self.W, self.out_size, *dzi, out=self.xf)
            PC, self.status = pc_sample.train_batch_to_pcl(self.depth, self.labels, self.inst_ids, self.xf, None, self.K,
                                                           n_pts=self.n_pts, out_size=self.out_size, min_pts=min_pts,
                                                           mask_pro=mask_pro, sampler=self.sampler)
            self.batch = pc_sample.train_batch_select(PC, self.status, self.keep, self.items, sel=self.sel, info=self.info)[0]
            return self.batch

        shapes = {"PC": torch.empty(self.keep, self.n_pts, 3, device=dev)}
        shapes.update({k: torch.empty((self.keep,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev) for k, v in self.items.items()})
        if self.draws is None:
            self._windows()
        state = self.sampler.get_state()                        # (the eager warm-up calls advance; the captured call does not)
        self.graphed = GraphedTrainStep(network, optimizer, shapes, scheduler=scheduler, max_norm=max_norm, warmup=warmup,
                                        prologue=front_end, draws=self.draws or "host",
                                        apply=apply, horizon=horizon, gate_info=self.info if apply == "graph" else None,
                                        accumulate=accumulate, global_step=global_step)
        self.sampler.set_state(state)

    def _scene(self):
        """what the captured prologue begins with: nothing here -- the frames are loaded (``RenderedTrainStep`` draws them)"""

    @staticmethod
    def _K_rows(K):
        K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
        return np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)

    def _load_small(self, frames):
        dev = self.depth.device
        if "inst_ids" in frames:
            ids = frames["inst_ids"]
            ids = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
            pc_sample._upload(ids.reshape(self.M), np.int32, dev, out=self.inst_ids)
        if "K" in frames:
            pc_sample._upload(self._K_rows(frames["K"]), np.float64, dev, out=self.K)
        if "bboxes_xyxy" in frames:
            boxes = np.array(frames["bboxes_xyxy"])
            if boxes.shape != (self.M, 4):
                raise ValueError(f"FrameTrainStep: expects bboxes_xyxy ({self.M},4) on the host, got {boxes.shape}")
            self.bboxes = boxes
            if self.draws is not None:
                if not np.issubdtype(boxes.dtype, np.integer):
                    raise ValueError(f"FrameTrainStep: under device draws bboxes_xyxy expects integers, got {boxes.dtype}")
                if not (np.maximum(boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]) > 0).all():
                    raise ValueError("FrameTrainStep: every box of bboxes_xyxy needs a positive side (the crop scale)")
                pc_sample._upload(boxes, np.int32, dev, out=self.bboxes_d)

    def _windows(self):
        centers, scales = pc_sample.dzi_windows(self.bboxes, self.H, self.W)
        pc_sample._upload(pc_sample.roi_transform(centers, scales, self.out_size), np.float64, self.xf.device, out=self.xf)

    def load(self, frames=None, items=None):
        """copy the next M items into the static buffers: depth / labels / items device to device, inst_ids / K through the
        pinned ring, bboxes_xyxy kept on the host for the next ``run()``'s windows; any subset of the keys"""
        if frames is not None:
            for k, dst in (("depth", self.depth), ("labels", self.labels)):
                if k in frames:
                    dst.copy_(frames[k], non_blocking=True)
            self._load_small(frames)
        if items is not None:
            for k, v in items.items():
                self.items[k].copy_(v, non_blocking=True)

    @property
    def loss_dict(self):
        return self.graphed.loss_dict

    @property
    def total(self):
        return self.graphed.total

    def run(self, check=True):
        """one training step from the frames in the static buffers; see the class text for ``check``"""
        if self.draws is None:
            self._windows()
        self.sampler.advance()
        self.graphed.replay()
        if self.graphed.clock is not None:                      # apply='graph': the device decided inside the replay
            if not check:
                return True
            clock = self.graphed.clock
            return clock.applied_last() if self.graphed.accum is None else clock.taken_last()
        if check and bool((self.info[0] == 0) | torch.isnan(self.graphed.total).any()):
            self.graphed.skip()                                 # (under accumulation the slot still passes)
            return False
        self.graphed.apply()
        return True


class RenderedTrainStep(FrameTrainStep):
    """``FrameTrainStep`` under device draws whose M items are not loaded but DRAWN: the captured prologue begins with
    ``source.draw(M, key, out=<the step's static buffers>)`` (``render.SceneSource``: the scene under the replay's key, the
    model points, the render, the guarded label boxes), then ``hsp_dzi_windows`` on those boxes, ``train_batch_to_pcl`` and
    ``train_batch_select`` as there, then ``GraphedTrainStep``'s body.  ``run()`` is ``sampler.advance()`` and one replay, then
    ``FrameTrainStep``'s check and apply rules, word for word (``apply='graph'`` included: ``run(check=False)`` is then safe and
    never waits).  No generator of the host's is touched, nothing is uploaded but the key, nothing is read back unless ``check``
    asks; equal sampler states give equal steps.  ``sel``, ``info``, ``status`` and ``batch`` are ``FrameTrainStep``'s; ``scene``
    holds every static tensor of the drawn scene (``SceneSource.buffers``).  There is nothing to ``load``.

    An item whose label has no pixel in its frame (hidden behind a distractor, say) gets the guarded box (0, 0, 1, 1): its
    window is finite and empty, the front end rejects it by count and the selection moves on to a spare.

    The remaining arguments are ``FrameTrainStep``'s; the draws are always the device's, so ``DZI_TYPE`` other than 'uniform'
    raises as it does there."""

    def __init__(self, network, optimizer, source, M, keep, sampler=None, **kw):
        if "draws" in kw:
            raise ValueError("RenderedTrainStep: the draws are always the device's; pass sampler=")
        dev = source.meshes.device
        sampler = pc_sample.draws_only(pc_sample.resolve_sampler("device" if sampler is None else sampler, dev), "RenderedTrainStep")
        if sampler is None:
            raise ValueError("RenderedTrainStep: expects a device sampler")
        self.source, self.scene = source, source.buffers(M)
        frames, items = source.draw(M, sampler.key, out=self.scene)      # (eager: what the static buffers start from)
        super().__init__(network, optimizer, frames, items, keep, sampler=sampler, draws=sampler, **kw)

    def _scene(self):
        if self.scene["depth"] is not self.depth:                        # first call: draw into the step's own static buffers
            self.scene.update(depth=self.depth, labels=self.labels, bboxes_d=self.bboxes_d, inst_ids=self.inst_ids, **self.items)
        self.source.draw(self.M, self.sampler.key, out=self.scene)

    def load(self, frames=None, items=None):
        raise TypeError("RenderedTrainStep: the items are drawn inside the replay; there is nothing to load")
