"""In-process A/B of the tile backward's two schedules on the benchmark's step: the B = 16, N = 1028 fp32 step is captured twice,
once under hsp_rf_bwd_set_schedule(1) (legacy) and once under (0) (batched) -- a captured graph keeps the schedule it was captured
with -- and the two graphs are replayed in alternating blocks; prints the median step of every block.
    python tools/ab_rf_bwd_schedule.py [blocks=4] [steps=100]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from hs_pose_amd._lib import lib
from hs_pose_amd.config import FLAGS
from hs_pose_amd.FaceRecon import FaceRecon
from hs_pose_amd.graph import GraphedStep

blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 4
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
dev = torch.device("cuda:0")
FLAGS.reset(); FLAGS.train = 0
torch.manual_seed(0)
net = FaceRecon().to(dev).train()
centred, obj, dfeat = bench.make_inputs(16, 1028, dev, seed=0)
torch.manual_seed(1)
L = lib()
graphs = {}
for name, legacy in (("legacy", 1), ("batched", 0)):
    prev = L.hsp_rf_bwd_set_schedule(legacy)
    try:
        graphs[name] = GraphedStep(net, centred, obj, dfeat, flat_grads=False, split=False)
    finally:
        L.hsp_rf_bwd_set_schedule(prev)
for g in graphs.values():
    for _ in range(20): g.run()
torch.cuda.synchronize()
med = {k: [] for k in graphs}
for _ in range(blocks):
    for name, g in graphs.items():
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        evs[0].record()
        for i in range(steps):
            g.run()
            evs[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
        med[name].append(ms[steps // 2])
for name, v in med.items():
    print(f"{name}: median ms per step, per block: {' '.join(f'{x:.4f}' for x in v)}")
print(f"gain (smallest legacy - largest batched): {1e3 * (min(med['legacy']) - max(med['batched'])):.1f} us")
