"""The training step with the gate, the schedule and the optimizer launch INSIDE the replay (``apply='graph'`` on
``graph.GraphedTrainStep`` / ``train.FrameTrainStep``) against the host-applied step, bit for bit under ``FLAGS.reproducible``
with device draws -- each mode in a fresh child process (tests/_apply_in_replay_check.py) like tests/test_gpu_train_graph.py: a
capture must precede the network's first eager backward.  The default form's pinned calls stay with
tests/test_gpu_frame_train.py (mode ``calls`` of tests/_frame_train_check.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("mode", ["twin", "skip", "rejected", "unarmed", "resume", "calls"])
def test_step_applied_inside_the_replay(dev, mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_apply_in_replay_check.py"), mode], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
