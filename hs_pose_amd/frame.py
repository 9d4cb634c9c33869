"""Depth frame + detections -> poses: the evaluation loop's two halves per image on the device.

The reference's loop builds one 1028-point cloud per detected instance on the CPU (evaluation/load_data_eval.py:207-254) and then
runs the network and ``generate_RT`` on them (evaluation/evaluate.py:90-106).  ``FramePipeline`` chains the package's pieces for
both: ``pc_sample.roi_windows`` (host integers) -> the frame front end -> a ``graph.GraphedInference`` kept per instance count.

With the host sampler (the default, ``FLAGS.pc_sampler = 'host'``) the front end is ``pc_sample.frame_to_pcl``: two kernels on
the frame, one device->host copy of the counts, the sample draws on numpy's global generator.  Nothing can be captured around
it: its draws need the counts on the host.  With a device sampler (``sampler='device'`` or a ``pc_sample.DeviceSampler``) it is
``pc_sample.frame_to_pcl_device``: three kernels, issued eagerly ahead of the replay with nothing copied back, or -- with
``one_graph=True`` -- captured together with the network, so that a frame is a few small uploads and ONE replay.  What that
replay still takes from the host is the network's two Pool_layer permutations, drawn on the CPU generator before it; with
``draws='device'`` (or ``FLAGS.step_draws = 'device'``) they are keyed draws inside the replay under the sampler's key as well.

With ``sampler='fps'`` (``pc_sample.FpsSampler``) the middle kernel of the device front end is ``hsp_fps_ids``: the rows are the
farthest-point picks over each instance's candidates and nothing is drawn for the clouds, in any of the three forms.  Under
``FLAGS.pool_sampler = 'fps'`` the Pool_layers pick their rows inside the replay too, and a frame's poses are then a pure
function of depth, masks, boxes, classes and K: no generator, no key, no host draw.

``FrameTracker`` is the front end of a video stream: no masks and no boxes, the crop of every instance is decided by the pose
the previous frame's replay left on the device (``pc_sample.track_to_pcl_device``), and that state is kept by the replay itself
(``hsp_track_update``).  A tracked frame is one depth copy, one key upload (none under 'fps') and one replay; a detector is
needed to ``start()`` the tracks and to re-seed the lost ones, not per frame.
"""
import numpy as np
import torch

from . import ops, pc_sample
from .graph import GraphedInference


class _FrameGraph:
    """roi_compact -> sample_ids (under the 'fps' sampler: fps_ids) -> frame_to_pcl -> network -> generate_RT of one (instance
    count, frame shape, depth dtype, mask form) as one captured graph over static buffers: the frame, the masks (or the label
    image and its ids), the crop transforms, K, the class rows and the sampler's key (the 'fps' sampler has none).  Everything
    is issued on the capture stream, in order; the kernels' workspaces and outputs come from the capture's pool."""

    def __init__(self, pipe, sampler, depth, masks, ids, xf, K, obj_id, n_pts, O, draws=None):
        dev = depth.device
        self.depth, self.masks = depth.clone(), masks.clone()
        self.ids = None if ids is None else pc_sample._upload(ids, np.int32, dev)
        self.xf = pc_sample._upload(xf, np.float64, dev)
        self.K = pc_sample._upload(K, np.float64, dev)
        self.obj_id = pc_sample._upload(obj_id, np.int64, dev)
        self.status = None
        key = sampler.key
        pipe._stand_in_cloud(n_pts, dev)                         # (made here: an upload cannot happen inside the capture)

        def front_end():
            src, count = ops.roi_compact(self.depth, self.masks, self.xf, O, self.ids)
            choose, self.status = pc_sample.choose_rows(sampler, key, self.depth, self.K, src, count, n_pts, pipe.min_pts)
            return pipe._network_input(ops.frame_to_pcl(self.depth, self.K, src, choose), self.status)

        n = xf.shape[0]
        self.graphed = GraphedInference(pipe.net, torch.empty(n, n_pts, 3, device=dev), self.obj_id,
                                        pipe.mean_shapes[self.obj_id], pipe.sym_infos[self.obj_id], prologue=front_end,
                                        draws=draws or "host")

    def load(self, pipe, depth, masks, ids, xf, K, obj_id):
        dev = depth.device
        self.depth.copy_(depth, non_blocking=True)
        self.masks.copy_(masks, non_blocking=True)
        if ids is not None:
            pc_sample._upload(ids, np.int32, dev, out=self.ids)
        pc_sample._upload(xf, np.float64, dev, out=self.xf)
        pc_sample._upload(K, np.float64, dev, out=self.K)
        pc_sample._upload(obj_id, np.int64, dev, out=self.obj_id)
        self.graphed.load(mean_shape=pipe.mean_shapes[self.obj_id], sym=pipe.sym_infos[self.obj_id])


class FramePipeline:
    """``pipe = FramePipeline(network, mean_shapes, sym_infos)`` with ``network`` an ``HSPose`` in eval() mode and the two
    per-class tables as device tensors: mean_shapes (C,3) fp32 metres (``get_mean_shape(...) / 1000``), sym_infos (C,4)
    (``get_sym_info``), row ``c`` for the detector's class id ``c + 1`` (the loader's ``cat_id_0base``).

    ``pipe(depth, masks, bboxes, class_ids, K) -> (pred_RT (n,4,4), pred_s (n,3))`` for depth (H,W) fp32 or uint16 mm and
    masks (n,H,W) uint8/bool on the device (or one (H,W) label image with ``inst_ids`` (n,)), bboxes (n,4) integer
    (y1, x1, y2, x2) and class_ids (n,) on the host (``pred_bboxes`` / ``pred_class_ids``), K (3,3).  Zero-row outputs for n = 0
    (evaluate.py:85-89); None when the front end rejects the frame (the loader returns None for it).  The outputs are the
    caller's (copies of the graph's static buffers).  The first frame with a new instance count captures its graph (a few ms,
    see GraphedInference).

    ``sampler``: None (follow ``FLAGS.pc_sampler`` at each call), 'host', 'device', a ``pc_sample.DeviceSampler`` or 'fps'.
    'fps' counts as a device sampler in everything below, with nothing to seed or advance: the rows of a cloud are picked by
    farthest-point sampling (``hsp_fps_ids``).  Under ``FLAGS.pool_sampler = 'fps'`` a frame then needs no key upload and no
    host draw and ``draws`` plays no part; under the default 'random' pool sampler the Pool_layers' rows are still drawn as
    ``draws`` says -- on the CPU generator before each replay, or keyed by the resolved ``draws`` sampler -- so the poses are
    deterministic only as far as those draws are.

    With a device sampler nothing is copied back before the poses: ``sync=True`` reads the per-instance status once, after
    everything is queued, and returns None for a rejected frame as above; ``sync=False`` never waits and returns
    ``(pred_RT, pred_s, status (n,) int32)`` as device tensors -- the rows of an instance whose status is not 0 mean nothing
    (the network ran on a stand-in cloud for it).  ``one_graph=True`` (device sampler only) captures the front end with the
    network: one graph per (instance count, frame shape, depth dtype, mask form), one replay per frame.

    ``draws``: None (follow ``FLAGS.step_draws`` at each call), 'host' -- the network's two Pool_layer permutations are drawn on
    the CPU generator before each replay --, 'device' or a DeviceSampler: they are drawn inside the replay, keyed by the
    pipeline's device sampler where it has one (one ``advance()`` per frame keys the cloud rows and the Pool rows alike), else by
    the resolved sampler.  With ``one_graph=True`` a frame's result is then a function of the static buffers and the key alone."""

    def __init__(self, network, mean_shapes, sym_infos, n_pts=None, out_size=None, min_pts=2, sampler=None, one_graph=False,
                 sync=True, draws=None):
        self.net, self.mean_shapes, self.sym_infos = network, mean_shapes, sym_infos
        self.n_pts, self.out_size, self.min_pts = n_pts, out_size, min_pts
        self.sampler, self.one_graph, self.sync, self.draws = sampler, bool(one_graph), bool(sync), draws
        self.graphs = {}                                         # instance count (device draws: and their sampler) -> GraphedInference
        self.frame_graphs = {}                                   # one_graph: (sampler, n, frame shape, dtype, ...) -> _FrameGraph

    def _network_input(self, PC, status):
        """the clouds the network is given: a rejected instance's rows are NaN by contract, and the neighbour search is not
        meant for those -- such an instance gets a fixed, well-spread stand-in cloud, its outputs are discarded or flagged"""
        return torch.where((status != 0)[:, None, None], self._stand_in_cloud(PC.shape[1], PC.device), PC)

    def _stand_in_cloud(self, n_pts, dev):
        return pc_sample.stand_in_cloud(n_pts, dev)

    def __call__(self, depth, masks, bboxes, class_ids, K, inst_ids=None):
        n = len(bboxes)
        dev = depth.device
        sampler = pc_sample.resolve_sampler(self.sampler, dev)
        if sampler is None and (self.one_graph or not self.sync):
            raise ValueError("FramePipeline: one_graph=True and sync=False need a device sampler (sampler='device', a DeviceSampler, "
                             "'fps', or FLAGS.pc_sampler = 'device' / 'fps'): the host draws wait for the counts")
        draws = pc_sample.resolve_draws(self.draws, dev)
        if draws is not None and isinstance(sampler, pc_sample.DeviceSampler):
            draws = sampler                                      # one key per frame (the 'fps' sampler has no key to share)
        if n == 0:
            out = torch.zeros(0, 4, 4, device=dev), torch.zeros(0, 3, device=dev)
            return out if self.sync else out + (torch.zeros(0, dtype=torch.int32, device=dev),)
        centers, scales = pc_sample.roi_windows(bboxes, depth.shape[0], depth.shape[1])
        if sampler is None:
            PC = pc_sample.frame_to_pcl(depth, masks, centers, scales, K, self.n_pts, self.out_size, inst_ids, self.min_pts, 'host')
            if PC is None:
                return None
            obj_id = torch.as_tensor(np.asarray(class_ids).astype(np.int64) - 1).to(dev, non_blocking=True)
            status = None
        elif self.one_graph:
            graphed, status = self._replay_frame(sampler, depth, masks, inst_ids, centers, scales, K, class_ids, draws)
            PC = None
        else:
            PC, status = pc_sample.frame_to_pcl_device(depth, masks, centers, scales, K, self.n_pts, self.out_size, inst_ids,
                                                       self.min_pts, sampler)
            PC = self._network_input(PC, status)
            obj_id = pc_sample._upload(np.asarray(class_ids).astype(np.int64) - 1, np.int64, dev)
        if PC is not None:                                       # the network's own graph, behind the eager front end
            mean_shape, sym = self.mean_shapes[obj_id], self.sym_infos[obj_id]
            slot = n if draws is None else (n, draws)
            graphed = self.graphs.get(slot)
            if graphed is None:
                graphed = self.graphs[slot] = GraphedInference(self.net, PC, obj_id, mean_shape, sym, draws=draws or "host")
            else:
                graphed.load(PC, obj_id, mean_shape, sym)
            if draws is not None and draws is not sampler:       # (the device front end has advanced its sampler for this frame)
                draws.advance()
            graphed.run()
        pred_RT, pred_s = graphed.pred_RT.clone(), graphed.pred_s.clone()
        if not self.sync:
            return pred_RT, pred_s, status.clone()
        if status is not None and bool(status.any()):            # the one wait of the device form, behind everything queued
            return None
        return pred_RT, pred_s

    def _replay_frame(self, sampler, depth, masks, inst_ids, centers, scales, K, class_ids, draws=None):
        n_pts, O, xf, masks, ids, K = pc_sample._frame_args(masks, centers, scales, K.cpu() if isinstance(K, torch.Tensor) else K,
                                                            self.n_pts, self.out_size, inst_ids)
        obj_id = np.asarray(class_ids).astype(np.int64) - 1
        key = (sampler, xf.shape[0], tuple(depth.shape), depth.dtype, masks.dim(), ids is None, K.shape[0], n_pts, O, draws)
        fg = self.frame_graphs.get(key)
        if fg is None:
            fg = self.frame_graphs[key] = _FrameGraph(self, sampler, depth, masks, ids, xf, K, obj_id, n_pts, O, draws)
        else:
            fg.load(self, depth, masks, ids, xf, K, obj_id)
        sampler.advance()
        if draws is not None and draws is not sampler:           # (the 'fps' sampler: the Pool rows' key is the draws sampler's)
            draws.advance()
        fg.graphed.run()
        return fg.graphed, fg.status


class _Tracks:
    """the static buffers of n tracked instances: the state the replays read and write (pose, size, frames lost), the class
    rows with their table rows, K by its row count"""

    def __init__(self, n, mean_shapes, sym_infos):
        dev = mean_shapes.device
        self.n = n
        self.RT = torch.zeros(n, 4, 4, device=dev)
        self.size = torch.zeros(n, 3, device=dev)
        self.lost = torch.zeros(n, dtype=torch.int32, device=dev)
        self.obj_id = torch.zeros(n, dtype=torch.int64, device=dev)
        self.mean_shape = torch.zeros((n,) + tuple(mean_shapes.shape[1:]), dtype=mean_shapes.dtype, device=dev)
        self.sym = torch.zeros((n,) + tuple(sym_infos.shape[1:]), dtype=sym_infos.dtype, device=dev)
        self.K, self.K_rows = {}, None

    def load_K(self, K):
        """K (3,3) or (n,3,3), host or device -> the static float64 buffer of its row count (made on first use)"""
        dev = self.RT.device
        if isinstance(K, torch.Tensor) and K.is_cuda:
            K = K.to(torch.float64).reshape(-1, 9)
        else:
            K = (K.detach().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)).astype(np.float64).reshape(-1, 9)
        rows = K.shape[0]
        if rows not in (1, self.n):
            raise ValueError(f"FrameTracker: expects K (3,3) or ({self.n},3,3), got {rows} rows")
        buf = self.K.get(rows)
        if buf is None:
            buf = self.K[rows] = torch.zeros(rows, 9, dtype=torch.float64, device=dev)
        if isinstance(K, torch.Tensor):
            buf.copy_(K, non_blocking=True)
        else:
            pc_sample._upload(K, np.float64, dev, out=buf)
        self.K_rows = rows


class _TrackGraph:
    """pose_windows -> roi_compact_box -> sample_ids (under the 'fps' sampler: fps_ids) -> frame_to_pcl -> stand-in where
    rejected -> network -> generate_RT -> pred_s -> track_update of one (instance count, frame shape, depth dtype, K rows) as one
    captured graph over static buffers: the frame (its own), the tracked state, K and the class rows (the ``_Tracks``') and the
    sampler's key.  The state is read by the head of the body and written by its tail: one stream, in order."""

    def __init__(self, trk, st, sampler, depth, n_pts, O, draws):
        dev = st.RT.device
        self.depth = torch.empty(tuple(depth.shape), dtype=depth.dtype, device=dev)
        self.depth.copy_(depth, non_blocking=True)
        self.status = None
        K, key, pad = st.K[st.K_rows], sampler.key, pc_sample.track_pad(trk.pad)
        pc_sample.stand_in_cloud(n_pts, dev)                     # (made here: an upload cannot happen inside the capture)

        def front_end():
            PC, self.status = pc_sample.track_chain(self.depth, st.RT, st.size, K, n_pts, O, trk.min_pts, pad, sampler, key)
            return _network_input(PC, self.status)

        def keep(g):
            ops.track_update(g.pred_RT, g.pred_s, self.status, st.RT, st.size, st.lost)

        state = st.RT.clone(), st.size.clone(), st.lost.clone()  # (the warm-up runs the body, and the body moves the state)
        self.graphed = GraphedInference(trk.net, torch.empty(st.n, n_pts, 3, device=dev), st.obj_id, st.mean_shape, st.sym,
                                        prologue=front_end, draws=draws or "host", epilogue=keep)
        for buf, was in zip((st.RT, st.size, st.lost), state):
            buf.copy_(was)


def _network_input(PC, status):
    """``FramePipeline._network_input``: the stand-in cloud where the front end rejected the instance"""
    return torch.where((status != 0)[:, None, None], pc_sample.stand_in_cloud(PC.shape[1], PC.device), PC)


class FrameTracker:
    """``trk = FrameTracker(network, mean_shapes, sym_infos)`` with the arguments of ``FramePipeline``: poses for a video
    stream with no mask and no box per frame.  The crop of instance j in frame t is decided by its pose and size after frame
    t - 1, which never leave the device (include/hsp.h: instances followed from frame to frame): the projection of the oriented
    box of half extents 0.5 * pad * size is the window, the box itself the mask.

    ``start(pred_RT, pred_s, class_ids)``: pred_RT (n,4,4) and pred_s (n,3) fp32 device tensors -- a ``FramePipeline``'s
    outputs for a frame with a detector's masks, say --, class_ids (n,) the detector's, on the host.  They are copied into the
    static state and every track's ``lost`` is 0; the class rows go up through the pinned ring.  A ``start()`` with an instance
    count seen before reuses its buffers and graphs: it is also the way to re-seed lost tracks.

    ``step(depth, K=None) -> (pred_RT (n,4,4), pred_s (n,3), status (n,) int32, lost (n,) int32)``, device tensors of the
    caller's; never waits.  depth (H,W) fp32 or uint16 mm, K (3,3) or (n,3,3) (None: the last one given).  One copy of the frame
    into its static buffer, ``sampler.advance()``, one replay: windows, box compaction, rows, clouds, stand-in where rejected,
    network, ``generate_RT``, ``pred_s = Pred_s + mean_shape``, ``hsp_track_update``.  status: bits 1 and 2 ``hsp_sample_ids``'s
    under ``min_pts`` (50: the training loader's rule), 4: the pose gave no window.  Where status is 0 the state takes the new
    pose and size and ``lost`` is 0; elsewhere the returned rows mean nothing (the network ran on a stand-in cloud), the state
    stays and ``lost`` counts the frames since.  One graph per (n, frame shape, depth dtype, K rows, sampler, draws), captured
    on first use.

    ``state() -> (RT (n,4,4), size (n,3), lost (n,))``: copies of the state, on the device.

    ``pad``: None follows ``FLAGS.DZI_PAD_SCALE`` (1.5, the padding the training crops are cut with).  ``sampler``: 'device', a
    ``pc_sample.DeviceSampler`` or 'fps' (None follows ``FLAGS.pc_sampler``); the host sampler is refused, its draws wait for
    the counts.  ``draws``: as ``FramePipeline``'s."""

    def __init__(self, network, mean_shapes, sym_infos, n_pts=None, out_size=None, min_pts=50, pad=None, sampler=None, draws=None):
        self.net, self.mean_shapes, self.sym_infos = network, mean_shapes, sym_infos
        self.n_pts, self.out_size, self.min_pts, self.pad = n_pts, out_size, int(min_pts), pad
        self.sampler, self.draws = sampler, draws
        self._sampler(mean_shapes.device)
        pc_sample.track_pad(pad)
        if self.min_pts < 1:
            raise ValueError(f"FrameTracker: expects min_pts >= 1, got {min_pts!r}")
        self.tracks, self.graphs, self._cur = {}, {}, None       # n -> _Tracks; (n, sampler, frame shape, ...) -> _TrackGraph

    def _sampler(self, dev):
        sampler = pc_sample.resolve_sampler(self.sampler, dev)
        if sampler is None:
            raise ValueError("FrameTracker: a tracked frame needs a device sampler (sampler='device', a DeviceSampler, 'fps', or "
                             "FLAGS.pc_sampler = 'device' / 'fps'): the host draws wait for the counts")
        return sampler

    def start(self, pred_RT, pred_s, class_ids):
        obj_id = np.asarray(class_ids).astype(np.int64).reshape(-1) - 1
        n = obj_id.shape[0]
        ok = n >= 1 and all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in (pred_RT, pred_s))
        if not ok or tuple(pred_RT.shape) != (n, 4, 4) or tuple(pred_s.shape) != (n, 3):
            raise ValueError(f"FrameTracker.start: expects pred_RT (n,4,4) and pred_s (n,3) fp32 on the device for n >= 1 "
                             f"class ids, got {tuple(getattr(pred_RT, 'shape', ()))}, {tuple(getattr(pred_s, 'shape', ()))}, n = {n}")
        if obj_id.min() < 0 or obj_id.max() >= self.mean_shapes.shape[0]:
            raise ValueError(f"FrameTracker.start: class ids expect 1 .. {self.mean_shapes.shape[0]}, got {list(class_ids)}")
        st = self.tracks.get(n)
        if st is None:
            st = self.tracks[n] = _Tracks(n, self.mean_shapes, self.sym_infos)
        st.RT.copy_(pred_RT.detach(), non_blocking=True)
        st.size.copy_(pred_s.detach(), non_blocking=True)
        st.lost.zero_()
        pc_sample._upload(obj_id, np.int64, st.RT.device, out=st.obj_id)
        st.mean_shape.copy_(self.mean_shapes[st.obj_id])
        st.sym.copy_(self.sym_infos[st.obj_id])
        self._cur = st

    def step(self, depth, K=None):
        st = self._cur
        if st is None:
            raise RuntimeError("FrameTracker.step: no track yet; start(pred_RT, pred_s, class_ids) first")
        dev = st.RT.device
        sampler = self._sampler(dev)
        draws = pc_sample.resolve_draws(self.draws, dev)
        if draws is not None and isinstance(sampler, pc_sample.DeviceSampler):
            draws = sampler                                      # one key per frame (the 'fps' sampler has no key to share)
        if K is not None:
            st.load_K(K)
        elif st.K_rows is None:
            raise ValueError("FrameTracker.step: the first frame of a track needs K")
        if not isinstance(depth, torch.Tensor) or depth.dim() != 2:
            raise ValueError(f"FrameTracker.step: expects depth (H,W), got {tuple(getattr(depth, 'shape', ()))}")
        n_pts = int(pc_sample.FLAGS.random_points if self.n_pts is None else self.n_pts)
        O = int(pc_sample.FLAGS.img_size if self.out_size is None else self.out_size)
        key = (st.n, sampler, tuple(depth.shape), depth.dtype, st.K_rows, n_pts, O, draws)
        tg = self.graphs.get(key)
        if tg is None:
            tg = self.graphs[key] = _TrackGraph(self, st, sampler, depth, n_pts, O, draws)
        else:
            tg.depth.copy_(depth, non_blocking=True)
        sampler.advance()
        if draws is not None and draws is not sampler:           # (the 'fps' sampler: the Pool rows' key is the draws sampler's)
            draws.advance()
        tg.graphed.run()
        return tg.graphed.pred_RT.clone(), tg.graphed.pred_s.clone(), tg.status.clone(), st.lost.clone()

    def state(self):
        st = self._cur
        if st is None:
            raise RuntimeError("FrameTracker.state: no track yet; start(pred_RT, pred_s, class_ids) first")
        return st.RT.clone(), st.size.clone(), st.lost.clone()
