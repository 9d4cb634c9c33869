"""Depth frame + detections -> poses: the evaluation loop's two halves per image on the device.

The reference's loop builds one 1028-point cloud per detected instance on the CPU (evaluation/load_data_eval.py:207-254) and then
runs the network and ``generate_RT`` on them (evaluation/evaluate.py:90-106).  ``FramePipeline`` chains the package's pieces for
both: ``pc_sample.roi_windows`` (host integers) -> ``pc_sample.frame_to_pcl`` (two kernels on the frame, one device->host copy of
the counts, the sample draws on numpy's global generator) -> a ``graph.GraphedInference`` kept per instance count.  Nothing is
captured around the front end: its draws need the counts on the host.
"""
import numpy as np
import torch

from . import pc_sample
from .graph import GraphedInference


class FramePipeline:
    """``pipe = FramePipeline(network, mean_shapes, sym_infos)`` with ``network`` an ``HSPose`` in eval() mode and the two
    per-class tables as device tensors: mean_shapes (C,3) fp32 metres (``get_mean_shape(...) / 1000``), sym_infos (C,4)
    (``get_sym_info``), row ``c`` for the detector's class id ``c + 1`` (the loader's ``cat_id_0base``).

    ``pipe(depth, masks, bboxes, class_ids, K) -> (pred_RT (n,4,4), pred_s (n,3))`` for depth (H,W) fp32 or uint16 mm and
    masks (n,H,W) uint8/bool on the device, bboxes (n,4) integer (y1, x1, y2, x2) and class_ids (n,) on the host
    (``pred_bboxes`` / ``pred_class_ids``), K (3,3).  Zero-row outputs for n = 0 (evaluate.py:85-89); None when
    ``frame_to_pcl`` rejects the frame (the loader returns None for it).  The outputs are the caller's (copies of the graph's
    static buffers).  The first frame with a new instance count captures its graph (a few ms, see GraphedInference)."""

    def __init__(self, network, mean_shapes, sym_infos, n_pts=None, out_size=None, min_pts=2):
        self.net, self.mean_shapes, self.sym_infos = network, mean_shapes, sym_infos
        self.n_pts, self.out_size, self.min_pts = n_pts, out_size, min_pts
        self.graphs = {}                                         # instance count -> GraphedInference

    def __call__(self, depth, masks, bboxes, class_ids, K):
        n = len(bboxes)
        dev = depth.device
        if n == 0:
            return torch.zeros(0, 4, 4, device=dev), torch.zeros(0, 3, device=dev)
        centers, scales = pc_sample.roi_windows(bboxes, depth.shape[0], depth.shape[1])
        PC = pc_sample.frame_to_pcl(depth, masks, centers, scales, K, self.n_pts, self.out_size, min_pts=self.min_pts)
        if PC is None:
            return None
        obj_id = torch.as_tensor(np.asarray(class_ids).astype(np.int64) - 1).to(dev, non_blocking=True)
        mean_shape, sym = self.mean_shapes[obj_id], self.sym_infos[obj_id]
        graphed = self.graphs.get(n)
        if graphed is None:
            graphed = self.graphs[n] = GraphedInference(self.net, PC, obj_id, mean_shape, sym)
        else:
            graphed.load(PC, obj_id, mean_shape, sym)
        pred_RT, pred_s, _ = graphed.run()
        return pred_RT.clone(), pred_s.clone()
