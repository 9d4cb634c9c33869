"""train.FrameTrainStep (frames with spares -> the kept items -> one training step, one hipGraph) against its twin, the
all-rejected batch, and GraphedTrainStep(prologue=None)'s unchanged call list.  Each case runs tests/_frame_train_check.py in a
fresh child process, like tests/test_gpu_train_graph.py: a capture must precede the network's first eager backward.

Measured on an MI355X (M = 6, keep = 4, N = 256; the child prints the worst relative differences): fp32 losses equal,
gradients within 1.7e-7 of the largest gradient, parameters after the step within 8e-17 -- not zero, so the bounds stay those of
tests/_train_graph_check.py; bf16 everything equal."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16", "rejected", "calls"])
def test_frame_train_step(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_frame_train_check.py"), "6", "4", "256", mode],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
