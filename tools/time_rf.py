"""event-timed rf_conv forward / backward and surface backward at the three level shapes (run on the GPU box); the backwards under
both schedules of the tile kernel (hsp_rf_bwd_set_schedule: legacy = 1, batched = 0), alternated three times in one process."""
import ctypes
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from hs_pose_amd import ops
from hs_pose_amd._lib import lib
dev = torch.device("cuda:0")
torch.manual_seed(0)
L = lib()


def timed(fn, reps=50):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def both_schedules(name, fn):
    prev = L.hsp_rf_bwd_set_schedule(0)
    try:
        t = {0: [], 1: []}
        for _ in range(3):
            for legacy in (1, 0):
                L.hsp_rf_bwd_set_schedule(legacy)
                t[legacy].append(timed(fn))
        print(f"{name}: legacy {min(t[1]):.1f} us ({' '.join(f'{v:.1f}' for v in t[1])})  batched {min(t[0]):.1f} us "
              f"({' '.join(f'{v:.1f}' for v in t[0])})")
    finally:
        L.hsp_rf_bwd_set_schedule(prev)


def vp(t): return ctypes.c_void_p(t.data_ptr())


# the three level shapes (all plan as pipelined forwards) and, forward only, one shape whose forward plans as plain (S = 8:
# the last column slot leaves no thread free for the next point's directions)
for B, N, C, k, S in ((16, 1028, 128, 20, 7), (16, 257, 256, 20, 7), (16, 64, 512, 8, 7), (16, 1028, 128, 20, 8)):
    SC = S * C
    pipelined = ctypes.c_int(0)
    L.hsp_rf_fwd_plan(k, S, C, ctypes.byref(pipelined))
    xyz = torch.randn(B, N, 3, device=dev)
    X = torch.relu(torch.randn(B, N, C, device=dev))
    fm = torch.randn(B, N, (S + 1) * C, device=dev)
    dirs = torch.randn(3, SC, device=dev)
    g = torch.randn(B, N, C, device=dev)
    idx = ops.knn(X, k)
    out, arg, fwin = ops._rf_conv_fwd_raw(xyz, idx, dirs, fm, S, True)
    saved = fwin if fwin is not None else fm
    def fwd(): ops._rf_conv_fwd_raw(xyz, idx, dirs, fm, S, True)
    def bwd(): ops._rf_conv_bwd_raw(xyz, idx, dirs, saved, arg, g, S)
    print(f"rf_conv fwd B{B} N{N} C{C} S{S} ({'pipelined' if pipelined.value else 'plain'}): {timed(fwd):.1f} us")
    if S != 7:
        continue
    both_schedules(f"rf_conv bwd B{B} N{N} C{C}", bwd)
    if N == 1028:                                        # the surface layer runs on the first level only
        sarg = torch.empty(B, N, SC, dtype=torch.int16, device=dev)
        sout = torch.empty(B, N, C, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.hsp_rf_surface_fwd(vp(xyz), vp(idx), vp(dirs), B, N, k, S, C, vp(sout), vp(sarg), st) == 0
        wsb = L.hsp_rf_bwd_scatter_workspace_bytes(B, SC)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        gd = torch.empty(3, SC, device=dev)
        def sbwd(): assert L.hsp_rf_surface_bwd(vp(xyz), vp(dirs), vp(sarg), vp(g), B, N, S, C, vp(gd), vp(ws), wsb, st) == 0
        both_schedules(f"rf_surface bwd B{B} N{N} K{C}", sbwd)
