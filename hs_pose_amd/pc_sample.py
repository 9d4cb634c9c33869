"""Depth map -> sampled object point cloud; mirror of network/point_sample/pc_sample.py:8-77.

``PC_sample(obj_mask, Depth, camK, coor2d)`` keeps the reference's signature, host RNG consumption
(one ``np.random.choice(l_all, samplenum, replace=l_all < samplenum)`` per image, in image order, on
numpy's global generator) and return convention (``(None, None)`` as soon as an image has <= 1 valid
pixel -- pc_sample.py:59-60).  The device work is two launches for the whole batch
(``hsp_pc_compact`` / ``hsp_pc_gather``, csrc/frontend.hip) with ONE device->host copy (the per-image
valid-pixel counts the host needs before it can draw) instead of the reference's per-image chain of
H x W maps, boolean-index compactions and implicit syncs.

``frame_to_pcl`` is the step in front of that for a whole camera frame: the evaluation loader's per-instance crop chain
(evaluation/load_data_eval.py:207-254 -- ``get_bbox``, three ``cv2.warpAffine(INTER_NEAREST)`` over the frame, the two validity
sums, ``_depth_to_pcl`` and ``_sample_points``) on a frame that is uploaded once: ``roi_window`` on the host, then
``hsp_roi_compact`` / ``hsp_frame_to_pcl`` (two stages, ONE device->host copy of the counts in between, the draws on numpy's
global generator like ``_sample_points``).  The crops themselves are never built.

Who draws is a switch: ``sampler=`` on the three functions, by default ``FLAGS.pc_sampler``.  ``'host'`` (the default) is all of
the above, draw for draw.  ``'device'`` -- or a ``DeviceSampler`` of one's own -- draws the rows between the two stages with
``hsp_sample_ids`` from a seeded counter-based generator: the same DISTRIBUTION (a uniform subset without replacement when long,
tiling or a uniform draw with replacement when short), not the same draws; the counts stay on the device, nothing is copied
back and nothing waits until the caller reads the result, and numpy's generator is never touched.  ``frame_to_pcl_device`` is
that form bare: clouds and per-instance status, both on the device.  ``'fps'`` -- the ``FpsSampler`` -- is the frame front end's
alone (``frame_to_pcl``, ``frame_to_pcl_device``, ``frame.FramePipeline``): no draw at all, the rows are picked between the two
stages by farthest-point sampling over each instance's back-projected candidates (``hsp_fps_ids``), a pure function of the
frame, the masks, the windows and K.  ``PC_sample``, ``depth_to_pcl`` and the training front end refuse it: there the sampling
noise is part of what the reference trains and evaluates with.

``dzi_windows`` + ``train_batch_to_pcl`` are the training loader's chain (datasets/load_data.py:228-278) for a batch of items,
each with its own frame: ``aug_bbox_DZI``'s windows on the host, draw for draw, then the crops, ``defor_2D``'s perturbation of
the cropped mask, the three rejection tests, the cloud and its rows on the device (``hsp_roi_defor`` / ``hsp_crop_compact`` /
``hsp_sample_ids`` / ``hsp_frames_to_pcl``), under a device sampler only.  ``train_batch_select`` is the loader's answer to a
rejected item behind it -- move on to the next index (:254-278) -- for a batch that arrives with spares: the first ``keep`` good
items and every per-item tensor of theirs in one launch (``hsp_batch_select``), nothing read back.

``resolve_draws`` / ``draw_scope`` are the switch for the OTHER draws of a forward or a replay -- the Pool_layers' kept rows, the
augmentation's uniforms and jitter, the DZI windows: ``FLAGS.step_draws`` 'host' (default: torch's and numpy's generators, as
the reference) or 'device' (keyed by a ``DeviceSampler``, drawn inside the forward or the captured body; include/hsp.h: "keyed
draws of a step").  One ``advance()`` keys everything one forward or replay draws.
"""
import contextlib

import numpy as np
import torch

from . import ops, staging
from .config import FLAGS

_U64 = (1 << 64) - 1


class DeviceSampler:
    """The key of the device draws (include/hsp.h: hsp_sample_ids): a seed and a call counter, two uint64 in a device buffer
    the kernel reads -- so a captured launch sees each replay's values -- and their host copy.  ``advance()`` once per sampling
    launch or replay: it queues the upload of (seed, counter) from pinned memory on the current stream without blocking (the
    pattern of ``graph.upload_pool_indices``) and bumps the counter; the launch that follows draws under that pair.  Equal
    states give equal draws: ``get_state()`` / ``set_state()`` / ``manual_seed()`` (counter back to 0)."""

    def __init__(self, seed, device):
        self.device = torch.device(device)
        self.key = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.manual_seed(seed)

    def manual_seed(self, seed):
        self.seed, self.calls = int(seed) & _U64, 0
        return self

    def get_state(self):
        """(seed, counter): the pair the next ``advance()`` uploads"""
        return self.seed, self.calls

    def set_state(self, state):
        self.seed, self.calls = int(state[0]) & _U64, int(state[1]) & _U64

    def advance(self):
        words = [w - (1 << 64) if w >> 63 else w for w in (self.seed, self.calls)]      # the uint64 bits in an int64 buffer

        def fill(pinned):
            pinned[0], pinned[1] = words
        if self.device.type == "cuda":
            staging.upload(fill, (2,), torch.int64, self.device, out=self.key)
        else:                                                    # (a host-side key: for inspection, the kernels are GPU-only)
            fill(self.key)
        self.calls = (self.calls + 1) & _U64
        return self.key


class FpsSampler:
    """The sampler that draws nothing: the rows an instance keeps are the farthest-point picks over its candidates
    (include/hsp.h: hsp_fps_ids_*).  No seed, no key, no state; ``advance()`` is there for the callers that advance a sampler
    once per frame and does nothing.  One object serves every device (``FPS``); it hashes by identity like a DeviceSampler, so
    it keys a graph cache the same way."""
    key = None

    def advance(self):
        return None

    def __repr__(self):
        return "FpsSampler()"


FPS = FpsSampler()


_default_samplers = {}


def default_sampler(device):
    """the module's sampler of ``device``, made on first use and seeded from ``torch.initial_seed()`` (never from a draw on
    numpy's generator: the device form leaves that generator alone)"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    s = _default_samplers.get(device)
    if s is None:
        s = _default_samplers[device] = DeviceSampler(torch.initial_seed(), device)
    return s


def resolve_sampler(sampler, device):
    """``sampler=`` of the front ends -> None (the host draws), a DeviceSampler or the FpsSampler: None follows
    ``FLAGS.pc_sampler``, 'host', 'device' (the module's default sampler), 'fps' (``FPS``), or a sampler object"""
    if sampler is None:
        sampler = getattr(FLAGS, "pc_sampler", "host")
    if isinstance(sampler, (DeviceSampler, FpsSampler)):
        return sampler
    if sampler == "host":
        return None
    if sampler == "device":
        return default_sampler(device)
    if sampler == "fps":
        return FPS
    raise ValueError(f"pc sampler: expects 'host', 'device', 'fps', a DeviceSampler or the FpsSampler, got {sampler!r}")


def draws_only(sampler, who):
    """``sampler`` as resolved, for a front end whose sampling noise is part of its contract: the 'fps' sampler is refused"""
    if isinstance(sampler, FpsSampler):
        raise ValueError(f"{who}: the 'fps' sampler is the frame front end's (frame_to_pcl, frame_to_pcl_device, FramePipeline); "
                         "here the rows are drawn: 'host', 'device' or a DeviceSampler")
    return sampler


def resolve_draws(draws, device):
    """``draws=`` of the forwards and captured steps -> None (the host draws: torch's and numpy's generators, as the reference)
    or the DeviceSampler that keys every draw of a forward or a replay on the device: None follows ``FLAGS.step_draws``, 'host',
    'device' (the module's default sampler), or a DeviceSampler"""
    if draws is None:
        draws = getattr(FLAGS, "step_draws", "host")
    if isinstance(draws, DeviceSampler):
        return draws
    if draws == "host":
        return None
    if draws == "device":
        return default_sampler(device)
    raise ValueError(f"step draws: expects 'host', 'device' or a DeviceSampler, got {draws!r}")


class _DrawScope:
    """the device draws of ONE forward: the sampler whose key they read, and the Pool_layers' rows (drawn for both levels by
    the first layer that asks, handed to the second)"""

    def __init__(self, sampler):
        self.sampler, self.key = sampler, sampler.key
        self._rows, self._asked = [], False

    def pool_rows(self, n, rate, levels=None):
        """the rows a Pool_layer keeps of ``n`` at ``rate``: level 0 for the first layer of the forward, level 1 for a second
        one that pools what the first kept.  ``levels`` = 2: both at once -> [rows0, rows1]"""
        if levels == 2:
            self._asked = True
            return ops.pool_rows_draw(self.key, n, rate, 2)
        if self._rows and self._rows[0][0] == (n, rate):
            return self._rows.pop(0)[1]
        if self._asked:
            raise ValueError("device draws: the Pool_layers of one forward are two at most, the second pooling the rows the "
                             "first kept at the same rate (include/hsp.h: hsp_pool_rows_draw)")
        self._asked = True
        m = n // rate
        if m // rate >= 1:
            rows0, rows1 = ops.pool_rows_draw(self.key, n, rate, 2)
            self._rows.append(((m, rate), rows1))
            return rows0
        return ops.pool_rows_draw(self.key, n, rate, 1)[0]


_draw_scope = None


@contextlib.contextmanager
def draw_scope(draws, device):
    """The scope of one forward's draws.  Under device draws (``resolve_draws``) it yields the ``_DrawScope`` every draw of the
    forward is keyed by and ``active_draws()`` returns it inside; under host draws it yields None.  The outermost scope of an
    eager forward advances the sampler once; a scope opened during a graph capture never does (the owner of the captured body
    advances before each replay); a scope inside a scope is the outer one."""
    global _draw_scope
    if _draw_scope is not None:
        yield _draw_scope[0]
        return
    device = torch.device(device)
    sampler = resolve_draws(draws, device) if device.type == "cuda" else None
    scope = None
    if sampler is not None:
        if not torch.cuda.is_current_stream_capturing():
            sampler.advance()
        scope = _DrawScope(sampler)
    _draw_scope = (scope,)
    try:
        yield scope
    finally:
        _draw_scope = None


def active_draws():
    """the open scope's _DrawScope, or None: no scope is open or the host draws"""
    return _draw_scope[0] if _draw_scope is not None else None


def _gather_safe(choose, pix, HW):
    """``hsp_pc_gather`` / ``hsp_depth_to_pcl`` index ``pix`` with ``choose`` unchecked and a rejected row of ``choose`` is -1:
    point such rows at entry 0 and make entry 0 a pixel id where nothing was compacted (only then is it out of range)."""
    pix[:, 0].clamp_(0, HW - 1)
    return choose.clamp_(min=0)


def PC_sample(obj_mask, Depth, camK, coor2d, sampler=None):
    """obj_mask (bs,1,H,W) (or (bs,2,H,W) mask logits), Depth (bs,1,H,W) in mm, camK (bs,3,3),
    coor2d (bs,2,H,W) pixel coordinates -> PC (bs, FLAGS.random_points, 3) in metres.  ``sampler``: see the module text; the
    device form reads the rejection status once everything is queued."""
    if obj_mask.shape[1] == 2:                                 # predicted mask (pc_sample.py:16-18)
        # argmax(softmax(m)) == argmax(m); first index on ties like torch.max
        obj_mask = (obj_mask[:, 1] > obj_mask[:, 0])
    if getattr(FLAGS, "sample_method", "basic") != "basic":    # pc_sample.py:68-70
        raise NotImplementedError
    samplenum = int(FLAGS.random_points)
    bs, H, W = Depth.shape[0], Depth.shape[2], Depth.shape[3]
    mask = obj_mask.reshape(bs, H * W).float()
    pix, count = ops.pc_compact(mask, Depth.reshape(bs, H * W))
    sampler = draws_only(resolve_sampler(sampler, Depth.device), "PC_sample")
    if sampler is not None:
        choose_d, status = ops.sample_ids(count, samplenum, sampler.advance(), 2, 0, 1)
        pc = ops.pc_gather(Depth.reshape(bs, H * W), coor2d.reshape(bs, 2, H * W), camK, pix,
                           _gather_safe(choose_d, pix, H * W))
        return (None, None) if bool(status.any()) else pc
    counts = count.cpu().numpy()                               # the one sync of the front end
    choose = np.empty((bs, samplenum), dtype=np.int32)
    for i in range(bs):
        l_all = int(counts[i])
        if l_all <= 1.0:
            return None, None
        choose[i] = np.random.choice(l_all, samplenum, replace=l_all < samplenum)
    choose_d = torch.from_numpy(choose).to(Depth.device, non_blocking=True)
    return ops.pc_gather(Depth.reshape(bs, H * W), coor2d.reshape(bs, 2, H * W), camK, pix, choose_d)


def sample_point_ids(total_pts_num, n_pts):
    """row ids PoseDataset._sample_points keeps (load_data.py:308-320): tile when short, a
    ``np.random.permutation`` prefix when long (same global-RNG consumption), identity otherwise."""
    if total_pts_num < n_pts:
        base = np.arange(total_pts_num)
        return np.concatenate([np.tile(base, n_pts // total_pts_num), base[:n_pts % total_pts_num]])
    if total_pts_num > n_pts:
        return np.random.permutation(total_pts_num)[:n_pts]
    return np.arange(total_pts_num)


def depth_to_pcl(depth, K, xymap, mask, n_pts=None, min_pts=50, sampler=None):
    """Batched mirror of the loader's cloud extraction: ``_depth_to_pcl(depth, K, xymap, mask) / 1000.0``
    (load_data.py:275, :322-333), the ``len(pcl_in) < 50`` rejection (:276) and ``_sample_points`` (:278).

    depth (B,1,H,W) or (B,H,W) fp32 mm, K (3,3) or (B,3,3) (float64 like the loader's intrinsics),
    xymap (B,2,H,W), mask (B,1,H,W) -> (B,n_pts,3) fp32 metres, or None if any image has < min_pts
    valid pixels (the loader skips such an item).  n_pts defaults to FLAGS.random_points.  ``sampler``: see the module text."""
    n_pts = int(FLAGS.random_points if n_pts is None else n_pts)
    B = depth.shape[0]
    HW = depth[0].numel()
    d = depth.reshape(B, HW).float()
    K64 = torch.as_tensor(K, dtype=torch.float64, device=depth.device).reshape(-1, 9)
    if K64.shape[0] == 1 and B > 1:
        K64 = K64.expand(B, 9)
    pix, count = ops.pc_compact(mask.reshape(B, HW).float(), d)
    sampler = draws_only(resolve_sampler(sampler, depth.device), "depth_to_pcl")
    if sampler is not None:
        choose_d, status = ops.sample_ids(count, n_pts, sampler.advance(), min_pts, 0, 0)
        pc = ops.depth_to_pcl(d, xymap.reshape(B, 2, HW), K64.contiguous(), pix, _gather_safe(choose_d, pix, HW))
        return None if bool(status.any()) else pc
    counts = count.cpu().numpy()
    choose = np.empty((B, n_pts), dtype=np.int32)
    for i in range(B):
        if int(counts[i]) < min_pts:
            return None
        choose[i] = sample_point_ids(int(counts[i]), n_pts)
    choose_d = torch.from_numpy(choose).to(depth.device, non_blocking=True)
    return ops.depth_to_pcl(d, xymap.reshape(B, 2, HW), K64.contiguous(), pix, choose_d)


def roi_window(bbox, im_H, im_W):
    """The square crop window of a detection: ``get_bbox`` (tools/eval_utils.py:159-187, its hard-wired 480 x 640 frame
    included) followed by load_data_eval.py:221-228.  bbox = (y1, x1, y2, x2) integers -> (center (2,) float32 = (cx, cy),
    scale float).  Integer arithmetic only: the window's corners are integers, so the centre is an integer or a half."""
    y1, x1, y2, x2 = (int(v) for v in bbox)
    if (y1, x1, y2, x2) != tuple(bbox):
        raise ValueError(f"roi_window: expects an integer box (y1, x1, y2, x2), got {tuple(bbox)}")
    half = min((max(y2 - y1, x2 - x1) // 40 + 1) * 40, 440) // 2
    rmin, rmax = (y1 + y2) // 2 - half, (y1 + y2) // 2 + half
    cmin, cmax = (x1 + x2) // 2 - half, (x1 + x2) // 2 + half
    if rmin < 0:
        rmin, rmax = 0, rmax - rmin
    if cmin < 0:
        cmin, cmax = 0, cmax - cmin
    if rmax > 480:
        rmin, rmax = rmin - (rmax - 480), 480
    if cmax > 640:
        cmin, cmax = cmin - (cmax - 640), 640
    scale = min(max(rmax - rmin, cmax - cmin), max(int(im_H), int(im_W)))
    return np.array([(cmin + cmax) * 0.5, (rmin + rmax) * 0.5], dtype=np.float32), float(scale)


def roi_windows(bboxes, im_H, im_W):
    """``roi_window`` of every row of bboxes (n,4) -> (centers (n,2) float32, scales (n,) float64)."""
    wins = [roi_window(tuple(np.asarray(b).tolist()), im_H, im_W) for b in bboxes]
    centers = np.stack([w[0] for w in wins]) if wins else np.zeros((0, 2), np.float32)
    return centers, np.array([w[1] for w in wins], dtype=np.float64)


def roi_transform(centers, scales, out_size):
    """(n,3) float64 rows (m0, b1, b2): the inverse of ``crop_resize_by_warp_affine``'s matrix with rot = 0
    (tools/dataset_utils.py:80-135), in the order of operations include/hsp.h fixes (every step one float64 rounding)."""
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 2)
    s = np.asarray(scales, dtype=np.float64).reshape(-1)
    if c.shape[0] != s.shape[0] or not (np.isfinite(c).all() and np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("roi_transform: expects n finite centres (n,2) and n finite scales > 0")
    O = float(out_size)
    a = O / s
    tx = O / 2 - a * c[:, 0]
    ty = O / 2 - a * c[:, 1]
    D = 1.0 / (a * a)
    m0 = a * D
    return np.stack([m0, -m0 * tx, -m0 * ty], axis=1)


def _upload(a, dtype, dev, out=None):
    """a small host array -> the device (into ``out`` when given) through the pinned ring (staging.py): queued behind the
    stream, not waited for"""
    a = np.ascontiguousarray(a, dtype=dtype)
    t = torch.from_numpy(a)
    return staging.upload(lambda pinned: pinned.copy_(t), t.shape, t.dtype, dev, out=out)


def _frame_args(masks, centers, scales, K, n_pts, out_size, inst_ids):
    """what every form of the frame front end makes of its arguments before anything goes to the device -> (n_pts, O, xf (n,3)
    float64, masks as uint8, ids (n,) int32 or None, K float64 (1|n, 9)), numpy's; a K that is on the device is left as given"""
    n_pts = int(FLAGS.random_points if n_pts is None else n_pts)
    O = int(FLAGS.img_size if out_size is None else out_size)
    xf = roi_transform(centers, scales, O)
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    ids = None if inst_ids is None else np.asarray(inst_ids).astype(np.int32)
    if not (isinstance(K, torch.Tensor) and K.is_cuda):
        K = (K.detach().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)).astype(np.float64).reshape(-1, 9)
    return n_pts, O, xf, masks, ids, K


def frame_to_pcl_device(depth, masks, centers, scales, K, n_pts=None, out_size=None, inst_ids=None, min_pts=2, sampler=None):
    """``frame_to_pcl`` with the rows chosen on the device: the same arguments, ``sampler`` a DeviceSampler (None or 'device':
    the module's) or 'fps' / the FpsSampler -> (PC (n, n_pts, 3) fp32 metres, status (n,) int32), both on the device.  status
    bit 0: fewer than min_pts crop pixels with depth and mask; bit 1: <= 1 with depth; the rows of such an instance are NaN and
    the frame is one the loader skips.  Three launches and the uploads of the small host arrays, all queued: no device->host
    copy, no wait.  Under 'fps' the middle launch is ``hsp_fps_ids`` in place of ``hsp_sample_ids``: nothing is drawn and no key
    goes up, the clouds are a function of the arguments alone."""
    n_pts, O, xf, masks, ids, K = _frame_args(masks, centers, scales, K, n_pts, out_size, inst_ids)
    dev = depth.device
    sampler = resolve_sampler("device" if sampler is None else sampler, dev)
    if sampler is None:
        raise ValueError("frame_to_pcl_device: expects a device sampler; the host draws are frame_to_pcl's")
    if xf.shape[0] == 0:
        return torch.zeros(0, n_pts, 3, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    ids_d = None if ids is None else _upload(ids, np.int32, dev)
    K64 = K.to(torch.float64).reshape(-1, 9).contiguous() if isinstance(K, torch.Tensor) else _upload(K, np.float64, dev)
    src, count = ops.roi_compact(depth, masks, _upload(xf, np.float64, dev), O, ids_d)
    choose, status = choose_rows(sampler, sampler.advance(), depth, K64, src, count, n_pts, min_pts)
    return ops.frame_to_pcl(depth, K64, src, choose), status


def choose_rows(sampler, key, depth, K64, src, count, n_pts, min_pts):
    """the middle launch of the frame front end -> (choose (n, n_pts) int32, status (n,) int32): ``hsp_fps_ids`` under the
    FpsSampler, else ``hsp_sample_ids`` under ``key`` (the sampler's, as advanced by the caller); the loader's two rejection
    tests either way"""
    if isinstance(sampler, FpsSampler):
        return ops.fps_ids(depth, K64, src, count, n_pts, min_pts, 2)
    return ops.sample_ids(count, n_pts, key, min_pts, 2, 0)


def track_pad(pad):
    """``pad=`` of the tracked front end -> the factor on the tracked size: None follows ``FLAGS.DZI_PAD_SCALE`` (1.5, the
    padding the training crops are cut with)"""
    pad = float(FLAGS.DZI_PAD_SCALE if pad is None else pad)
    if not 0.0 < pad < float("inf"):
        raise ValueError(f"track pad: expects a finite factor > 0, got {pad!r}")
    return pad


def track_chain(depth, RT, size, K64, n_pts, O, min_pts, pad, sampler, key):
    """the four launches of the tracked front end on device tensors alone (nothing uploaded, the sampler not advanced: ``key``
    is its key as the caller advanced it) -> (PC, status); what ``track_to_pcl_device`` issues and ``frame.FrameTracker``
    captures"""
    H, W = depth.shape
    _, xf, wstatus = ops.pose_windows(RT, size, K64, H, W, O, pad)
    src, count = ops.roi_compact_box(depth, RT, size, pad, K64, xf, O, wstatus)
    choose, status = choose_rows(sampler, key, depth, K64, src, count, n_pts, min_pts)
    return ops.frame_to_pcl(depth, K64, src, choose), status | wstatus


def track_to_pcl_device(depth, RT, size, K, n_pts=None, out_size=None, min_pts=50, pad=None, sampler=None):
    """``frame_to_pcl_device`` without masks and boxes: the crop of instance j is decided by its last pose.  depth (H,W) fp32
    or uint16 mm, RT (n,4,4) fp32 rigid poses in metres and size (n,3) fp32 metres on the device (what the previous frame's
    ``generate_RT`` and ``Pred_s + mean_shape`` left there), K (3,3) or (n,3,3) -> (PC (n, n_pts, 3) fp32 metres, status (n,)
    int32), both on the device.  The window is the projection of the oriented box of half extents 0.5 * pad * size about the
    pose, the mask is that box in metres (include/hsp.h: instances followed from frame to frame).  status: ``hsp_sample_ids``'s
    bits 1 and 2 under ``min_pts`` (50: the training loader's rule, load_data.py:276), plus 4: the pose gives no window (behind
    the camera, off the frame, not finite, a size <= 0); the rows of an instance whose status is not 0 are NaN.  ``pad``: None
    follows ``FLAGS.DZI_PAD_SCALE``.  ``sampler``: a DeviceSampler (None or 'device': the module's) or 'fps'.  Four launches --
    windows, compaction, rows, clouds --, all queued: nothing is copied back and nothing waits.  Inside a graph capture K must be
    a float64 device tensor and the sampler is not advanced (``sampler.advance()`` before each replay)."""
    n_pts = int(FLAGS.random_points if n_pts is None else n_pts)
    O = int(FLAGS.img_size if out_size is None else out_size)
    dev = depth.device
    sampler = resolve_sampler("device" if sampler is None else sampler, dev)
    if sampler is None:
        raise ValueError("track_to_pcl_device: expects a device sampler; the host draws wait for the counts")
    capturing = dev.type == "cuda" and torch.cuda.is_current_stream_capturing()
    if isinstance(K, torch.Tensor) and K.is_cuda:
        K64 = K.to(torch.float64).reshape(-1, 9).contiguous()
    elif capturing:
        raise ValueError("track_to_pcl_device: inside a graph capture K must already be on the device")
    else:
        K64 = _upload((K.detach().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)).reshape(-1, 9), np.float64, dev)
    key = sampler.key if capturing else sampler.advance()
    return track_chain(depth, RT, size, K64, n_pts, O, min_pts, track_pad(pad), sampler, key)


def frame_to_pcl(depth, masks, centers, scales, K, n_pts=None, out_size=None, inst_ids=None, min_pts=2, sampler=None):
    """The evaluation loader's crops and clouds for all detections of one frame (load_data_eval.py:230-254; with ``inst_ids``
    and ``min_pts=50`` the training loader's, datasets/load_data.py:234-278 without ``defor_2D``).

    depth (H,W) fp32 or uint16 mm on the device, masks uint8/bool (n,H,W) on the device -- or one (H,W) label image with
    inst_ids (n,) --, centers (n,2) / scales (n,) on the host (``roi_windows``, or the loader's DZI draws), K (3,3) or (n,3,3)
    -> (n, n_pts, 3) fp32 metres, or None if an instance has <= 1 crop pixels with depth or fewer than min_pts with depth and
    mask (the loader skips such a frame; decided before anything is drawn).  n_pts defaults to FLAGS.random_points, out_size to
    FLAGS.img_size.  One device->host copy; per instance, in order, the draws of ``sample_point_ids``.  ``sampler``: see the
    module text; the device and 'fps' forms are ``frame_to_pcl_device`` with its status read once everything is queued."""
    dsampler = resolve_sampler(sampler, depth.device)
    if dsampler is not None:
        PC, status = frame_to_pcl_device(depth, masks, centers, scales, K, n_pts, out_size, inst_ids, min_pts, dsampler)
        return None if bool(status.any()) else PC
    n_pts, O, xf, masks, ids, K = _frame_args(masks, centers, scales, K, n_pts, out_size, inst_ids)
    n = xf.shape[0]
    dev = depth.device
    if n == 0:
        return torch.zeros(0, n_pts, 3, dtype=torch.float32, device=dev)
    ids_d = None if ids is None else torch.from_numpy(ids).to(dev, non_blocking=True)
    K64 = torch.as_tensor(K, dtype=torch.float64).reshape(-1, 9).to(dev, non_blocking=True)
    src, count = ops.roi_compact(depth, masks, torch.from_numpy(xf).to(dev, non_blocking=True), O, ids_d)
    counts = count.cpu().numpy()                               # the one sync of the front end
    if (counts[:, 1] <= 1).any() or (counts[:, 0] < min_pts).any():
        return None
    choose = np.empty((n, n_pts), dtype=np.int32)
    for j in range(n):
        choose[j] = sample_point_ids(int(counts[j, 0]), n_pts)
    choose_d = torch.from_numpy(choose).to(dev, non_blocking=True)
    return ops.frame_to_pcl(depth, K64.contiguous(), src, choose_d)


def dzi_windows(bboxes_xyxy, im_H, im_W):
    """The crop windows of a training batch: ``aug_bbox_DZI`` (tools/dataset_utils.py:24-61) of every row of bboxes_xyxy (B,4)
    = (x1, y1, x2, y2) -> (centers (B,2) float64 = (cx, cy), scales (B,) float64).  With ``FLAGS.DZI_TYPE`` 'uniform' the
    reference's draws on numpy's global generator in its order -- per box one ``random_sample()``, then ``random_sample(2)`` --
    and its arithmetic, operation for operation; 'roi10d' and 'truncnorm' are not built; any other type gives the undrawn
    centre and side (the reference's ``else`` branch)."""
    kind = str(FLAGS.DZI_TYPE).lower()
    if kind in ("roi10d", "truncnorm"):
        raise NotImplementedError(f"dzi_windows: DZI_TYPE {FLAGS.DZI_TYPE!r} is not built ('uniform', or any other name for no draw)")
    boxes = np.asarray(bboxes_xyxy)
    if boxes.ndim != 2 or boxes.shape[1] != 4:
        raise ValueError(f"dzi_windows: expects boxes (B,4) = (x1, y1, x2, y2), got {boxes.shape}")
    centers, scales = np.zeros((len(boxes), 2), np.float64), np.zeros(len(boxes), np.float64)
    for k, (x1, y1, x2, y2) in enumerate(boxes):
        cx = 0.5 * (x1 + x2)
        cy = 0.5 * (y1 + y2)
        bh = y2 - y1
        bw = x2 - x1
        if kind == "uniform":
            scale_ratio = 1 + FLAGS.DZI_SCALE_RATIO * (2 * np.random.random_sample() - 1)
            shift_ratio = FLAGS.DZI_SHIFT_RATIO * (2 * np.random.random_sample(2) - 1)
            centers[k] = cx + bw * shift_ratio[0], cy + bh * shift_ratio[1]
            scale = max(y2 - y1, x2 - x1) * scale_ratio * FLAGS.DZI_PAD_SCALE
        else:
            centers[k] = cx, cy
            scale = max(y2 - y1, x2 - x1)
        scales[k] = min(scale, max(im_H, im_W)) * 1.0
    return centers, scales


def mask_gate(pro):
    """``defor_2D``'s ``rand_pro`` as the integer the kernel compares a 32-bit draw with (include/hsp.h: the mask rule):
    floor(pro * 2^32) clipped to [0, 2^32] -- 0 never deforms, 2^32 always does"""
    return int(min(max(np.floor(float(pro) * 4294967296.0), 0.0), 4294967296.0))


def train_batch_to_pcl(depth, labels, inst_ids, centers, scales, K, n_pts=None, out_size=None, min_pts=50, mask_pro=None,
                       mask_iters=1, sampler=None):
    """The training loader's crops, mask perturbation and clouds for a batch of items (datasets/load_data.py:234-278 behind
    ``aug_bbox_DZI``), all on the device: ``hsp_roi_defor`` -> ``hsp_crop_compact`` -> ``hsp_sample_ids`` ->
    ``hsp_frames_to_pcl``, a linear chain with no device->host copy and no wait.

    depth (B,H,W) -- a frame per item -- or (H,W), fp32 or uint16 mm on the device; labels uint8/bool on the device: (B,H,W) or
    (H,W) label images with inst_ids (B,), or with inst_ids None one mask per item (B,H,W); centers (B,2) / scales (B,) on the
    host (``dzi_windows``); K (3,3) or (B,3,3) -> (PC (B, n_pts, 3) fp32 metres, status (B,) int32), both on the device.
    status: ``hsp_sample_ids``'s bits -- 1: fewer than min_pts crop pixels with depth under the DEFORMED mask (:276), 2: <= 1
    with depth (:254) -- plus 4: <= 1 with depth under the mask BEFORE the deformation (:257).  The rows of an item whose
    status is not 0 are NaN: the loader skips such an item (``train_batch_select`` is that skip on the device).  mask_pro defaults to FLAGS.roi_mask_pro, n_pts to
    FLAGS.random_points, out_size to FLAGS.img_size; mask_iters is the rule's r, and 1 is what the reference's call runs
    whatever FLAGS.roi_mask_r says.

    The draws -- who is deformed, which band pixels go, which rows are kept -- are the device sampler's (None: the module's),
    one ``advance()`` per call: the reference's distributions, not its draws; numpy's generator is never touched.  There is no
    host-draw form: the reference interleaves the window, mask and row draws item by item.

    Inside ``torch.cuda.graph`` the call uploads nothing: give it inst_ids (B,) int32, the transform rows
    ``roi_transform(centers, scales, out_size)`` (B,3) float64 in place of centers with scales None, and K float64 as device
    tensors made before the capture; the sampler is not advanced by the captured call -- ``sampler.advance()`` before each replay,
    as ``frame._FrameGraph`` does."""
    n_pts = int(FLAGS.random_points if n_pts is None else n_pts)
    O = int(FLAGS.img_size if out_size is None else out_size)
    dev = depth.device
    sampler = draws_only(resolve_sampler("device" if sampler is None else sampler, dev), "train_batch_to_pcl")
    if sampler is None:
        raise ValueError("train_batch_to_pcl: expects a device sampler; there is no host-draw form of this chain")
    capturing = dev.type == "cuda" and torch.cuda.is_current_stream_capturing()

    def on_device(a, dtype, what):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a
        if capturing:
            raise ValueError(f"train_batch_to_pcl: inside a graph capture {what} must already be on the device")
        return _upload(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a), dtype, dev)

    if scales is None:
        xf = on_device(centers, np.float64, "the transform rows")
    else:
        xf = on_device(roi_transform(centers, scales, O), np.float64, "the transform rows (pass them as centers, scales=None)")
    ids_d = None if inst_ids is None else on_device(inst_ids, np.int32, "inst_ids")
    K64 = on_device(K, np.float64, "K").to(torch.float64).reshape(-1, 9)
    if labels.dtype == torch.bool:
        labels = labels.view(torch.uint8)
    gate = mask_gate(FLAGS.roi_mask_pro if mask_pro is None else mask_pro)
    scope = active_draws()                                      # (a forward's draw scope of this sampler has advanced it already)
    key = sampler.key if capturing or (scope is not None and scope.sampler is sampler) else sampler.advance()
    crop_mask, _ = ops.roi_defor(labels, xf, O, key, ids_d, mask_iters, gate)
    src, count, pre = ops.crop_compact(depth, crop_mask, xf, O)
    choose, status = ops.sample_ids(count, n_pts, key, min_pts, 2, 0)
    early = pre <= 1
    PC = ops.frames_to_pcl(depth, K64, src, torch.where(early[:, None], -1, choose))
    return PC, status | (early.to(torch.int32) << 2)


_stand_ins = {}


def stand_in_cloud(n_pts, device):
    """the fixed, well-spread cloud (n_pts, 3) the network is given where a front end rejected the real one (a rejected item's
    rows are NaN by contract, and the neighbour search is not meant for those): uniform in a 0.2 m cube about the origin, from
    a generator of its own seeded 0.  Kept per (n_pts, device); the first call uploads, so make it before a capture."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    c = _stand_ins.get((int(n_pts), device))
    if c is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise ValueError("stand_in_cloud: the first call for a size uploads the cloud; make it before the graph capture")
        g = torch.Generator().manual_seed(0)
        c = _stand_ins[(int(n_pts), device)] = ((torch.rand(int(n_pts), 3, generator=g) - 0.5) * 0.2).to(device)
    return c


def train_batch_select(PC, status, keep, extras, stand_in=None, out=None, sel=None, info=None):
    """The loader's "move on to the next index" (datasets/load_data.py:254-278) for a batch that arrives with spares, on the
    device: PC (M, n_pts, 3) and status (M,) int32 of ``train_batch_to_pcl``, extras a dict of per-item device tensors with
    leading dimension M (obj_id, gt_R, gt_t, gt_s, mean_shape, sym, aug_bb, aug_rt_t, aug_rt_r, model_point, nocs_scale, or any
    subset; at most 15) -> (batch, sel (keep,) int32, info (2,) int32): batch holds ``PC`` and every extra with leading dimension
    keep, the rows of the first keep items whose status is 0, in order -- sel names them; with fewer than keep good items the good
    ones repeat in order; info = [good items, min(good items, keep)] (include/hsp.h: hsp_batch_select).  No row of a rejected
    item reaches the batch.  With NO good item sel is the identity, the extras are rows 0 .. keep-1 and every cloud is
    ``stand_in`` (n_pts, 3) -- by default ``stand_in_cloud`` -- so that the network never sees NaN rows; info[0] == 0 says so.

    One ``ops.batch_select`` launch; nothing is uploaded or read back, so the call can be captured (a default stand-in must
    exist before the capture: call ``stand_in_cloud(n_pts, device)`` first).  The outputs are fresh tensors, or the caller's:
    ``out`` a dict with a contiguous tensor per key of batch (``PC`` included), ``sel`` / ``info`` int32 buffers."""
    if "PC" in extras:
        raise ValueError("train_batch_select: 'PC' is the cloud argument, not an extra")
    if PC.dim() != 3 or PC.shape[2] != 3:
        raise ValueError(f"train_batch_select: expects PC (M, n_pts, 3), got {tuple(PC.shape)}")
    if stand_in is None:
        stand_in = stand_in_cloud(PC.shape[1], PC.device)
    names = ["PC"] + list(extras)
    if out is not None and set(out) != set(names):
        raise ValueError(f"train_batch_select: out expects the keys {sorted(names)}, got {sorted(out)}")
    segs = [(PC if k == "PC" else extras[k], None if out is None else out[k], stand_in if k == "PC" else None) for k in names]
    dsts, sel, info = ops.batch_select(status, keep, segs, sel=sel, info=info)
    return dict(zip(names, dsts)), sel, info
