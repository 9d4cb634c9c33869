"""tools/gen_golden_train_frontend.py -- TEST INFRASTRUCTURE ONLY.  Runs ONLY in the build container (it imports the reference).

Golden crop windows for hs_pose_amd/pc_sample.py::dzi_windows: 64 boxes (x1, y1, x2, y2) on a 480 x 640 frame pushed, in order,
through the reference's own ``aug_bbox_DZI`` (tools/dataset_utils.py:24-61) under ``np.random.seed(0)`` with the reference's
flag defaults (DZI_TYPE 'uniform', ratios 0.25, pad 1.5), and once more with a type that draws nothing (the ``else`` branch).
Boxes, centres, scales and the generator's position afterwards go to tests/golden/train_dzi_windows.npz, their shapes and
dtypes to tests/golden/train_frontend_manifest.json: numeric arrays only.  Like tools/gen_golden_frame.py this must be run as
a script, so that ``tools`` resolves to the reference's package.

usage:  python tools/gen_golden_train_frontend.py
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]
sys.path[:0] = [os.path.join(ROOT, "oracle", "stubs"), REF]

import numpy as np  # noqa: E402

from tools.dataset_utils import aug_bbox_DZI  # noqa: E402

assert os.path.abspath(sys.modules["tools"].__path__[0]) == os.path.join(REF, "tools")

GOLD = os.path.join(ROOT, "tests", "golden")
IM_H, IM_W = 480, 640
SEED = 0


def boxes():
    rng = np.random.RandomState(31)
    out = []
    for _ in range(48):                                    # ordinary boxes
        h, w = rng.randint(8, 280), rng.randint(8, 280)
        y1, x1 = rng.randint(0, IM_H - h), rng.randint(0, IM_W - w)
        out.append((x1, y1, x1 + w, y1 + h))
    out += [(0, 0, 60, 45), (600, 0, 640, 30), (0, 440, 35, 480), (590, 430, 640, 480),       # frame corners and edges
            (0, 200, 12, 260), (628, 200, 640, 290), (300, 0, 380, 9), (300, 470, 420, 480),
            (0, 0, 640, 480), (10, 5, 630, 470), (-40, -30, 700, 520),                          # as large as, and larger than, the frame
            (100, 100, 101, 101), (320, 240, 320, 240), (5, 7, 6, 300), (7, 5, 500, 6), (200, 150, 520, 470)]
    assert len(out) == 64
    return np.array(out, dtype=np.int64)


def run(bb, dzi_type):
    flags = types.SimpleNamespace(DZI_TYPE=dzi_type, DZI_PAD_SCALE=1.5, DZI_SCALE_RATIO=0.25, DZI_SHIFT_RATIO=0.25)
    np.random.seed(SEED)
    centers, scales = [], []
    for b in bb:
        c, s = aug_bbox_DZI(flags, b, IM_H, IM_W)
        centers.append(np.asarray(c, dtype=np.float64))
        scales.append(float(s))
    st = np.random.get_state()
    return np.array(centers), np.array(scales, dtype=np.float64), st[1].astype(np.uint32), np.array([st[2]], dtype=np.int64)


def main():
    bb = boxes()
    c_u, s_u, keys_u, pos_u = run(bb, "uniform")
    c_n, s_n, keys_n, pos_n = run(bb, "none")
    arrs = dict(boxes=bb, im_hw=np.array([IM_H, IM_W], dtype=np.int32), seed=np.array([SEED], dtype=np.int64),
                centers_uniform=c_u, scales_uniform=s_u, state_keys_uniform=keys_u, state_pos_uniform=pos_u,
                centers_none=c_n, scales_none=s_n, state_keys_none=keys_n, state_pos_none=pos_n)
    print(f"{len(bb)} boxes; clamped to max(H, W): uniform {(s_u == max(IM_H, IM_W)).sum()}, none {(s_n == max(IM_H, IM_W)).sum()}; "
          f"generator position uniform {pos_u[0]}, none {pos_n[0]}")
    path = os.path.join(GOLD, "train_dzi_windows.npz")
    np.savez_compressed(path, **arrs)
    man = {"files": {"train_dzi_windows": {k: [list(v.shape), str(v.dtype)] for k, v in arrs.items()}}}
    with open(os.path.join(GOLD, "train_frontend_manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
