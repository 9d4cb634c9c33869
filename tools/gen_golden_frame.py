"""tools/gen_golden_frame.py -- TEST INFRASTRUCTURE ONLY.  Runs ONLY in the build container (it imports the reference).

Golden crop windows for hs_pose_amd/pc_sample.py::roi_window: ~200 integer detection boxes (y1, x1, y2, x2) on a 480 x 640
frame pushed through the reference's own ``get_bbox`` (tools/eval_utils.py:159-187); centre and scale then follow the loader's
own arithmetic on that window (evaluation/load_data_eval.py:221-228).  Boxes, windows, centres and scales go to
tests/golden/frame_roi_windows.npz, their shapes and dtypes to tests/golden/frame_manifest.json.  The reference is imported with the stubs under oracle/stubs/ for the packages the image
lacks; this script lives in a folder that is itself called ``tools``, so it must be run as a script (its folder, not the
repository root, is then on sys.path and ``tools`` resolves to the reference's package).

usage:  python tools/gen_golden_frame.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]
sys.path[:0] = [os.path.join(ROOT, "oracle", "stubs"), REF]

import numpy as np  # noqa: E402
import matplotlib.pyplot  # noqa: F401,E402

from tools.eval_utils import get_bbox  # noqa: E402

assert os.path.abspath(sys.modules["tools"].__path__[0]) == os.path.join(REF, "tools")

GOLD = os.path.join(ROOT, "tests", "golden")
IM_H, IM_W = 480, 640


def boxes():
    rng = np.random.RandomState(20)
    out = []
    for _ in range(140):                                   # ordinary detections
        h, w = rng.randint(1, 300), rng.randint(1, 300)
        y1, x1 = rng.randint(0, IM_H - h), rng.randint(0, IM_W - w)
        out.append((y1, x1, y1 + h, x1 + w))
    for k in range(10):                                    # windows that clamp at each of the four frame edges
        out += [(0, 100 + 30 * k, 10 + 7 * k, 160 + 30 * k), (470 - 7 * k, 100 + 30 * k, 479, 180 + 30 * k),
                (100 + 20 * k, 0, 150 + 20 * k, 9 + 5 * k), (100 + 20 * k, 630 - 5 * k, 170 + 20 * k, 639)]
    out += [(0, 0, 30, 45), (0, 600, 25, 639), (450, 0, 479, 33), (455, 610, 479, 639)]          # corners: two edges at once
    for k in range(8):                                     # the 440 cap (a side of 400 or more)
        out.append((5 * k, 10 * k, 5 * k + 400 + 9 * k, 10 * k + 380 + 30 * k))
    out += [(0, 0, 479, 639), (0, 0, 480, 640), (20, 100, 459, 539)]
    for k in range(6):                                     # sides 360 and 400
        out.append((10 + k, 20 + 40 * k, 10 + k + 325 + 13 * k, 20 + 40 * k + 300))
    for y, x in ((0, 0), (0, 639), (479, 0), (479, 639), (240, 320), (17, 333), (1, 1), (478, 638)):   # degenerate boxes
        out += [(y, x, y, x), (y, x, min(y + 1, 479), min(x + 1, 639))]
    return np.array(out, dtype=np.int32)


def main():
    bb = boxes()
    windows, centers, scales = [], [], []
    for b in bb:
        rmin, rmax, cmin, cmax = get_bbox(b)
        # load_data_eval.py:221-228 on the window the reference returned
        x1, y1, x2, y2 = np.array([cmin, rmin, cmax, rmax])
        centers.append(np.array([0.5 * (x1 + x2), 0.5 * (y1 + y2)]))
        scales.append(min(max(y2 - y1, x2 - x1), max(IM_H, IM_W)) * 1.0)
        windows.append((rmin, rmax, cmin, cmax))
    arrs = dict(boxes=bb, windows=np.array(windows, dtype=np.int32), centers=np.array(centers, dtype=np.float64),
                scales=np.array(scales, dtype=np.float64), im_hw=np.array([IM_H, IM_W], dtype=np.int32))
    w = arrs["windows"]
    side = w[:, 1] - w[:, 0]
    print(f"{len(bb)} boxes; sides {sorted(set(side.tolist()))}; clamped top {(w[:, 0] == 0).sum()} bottom {(w[:, 1] == IM_H).sum()} "
          f"left {(w[:, 2] == 0).sum()} right {(w[:, 3] == IM_W).sum()}; capped {(side == 440).sum()}")
    path = os.path.join(GOLD, "frame_roi_windows.npz")
    np.savez_compressed(path, **arrs)
    # shapes and dtypes, in the form of tests/golden/manifest.json, in a manifest of this fixture's own: that file belongs to the
    # generators under oracle/ and is left as they wrote it
    mpath = os.path.join(GOLD, "frame_manifest.json")
    man = {"files": {"frame_roi_windows": {k: [list(v.shape), str(v.dtype)] for k, v in arrs.items()}}}
    with open(mpath, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
