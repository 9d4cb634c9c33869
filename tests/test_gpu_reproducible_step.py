"""Whole training steps under ``FLAGS.reproducible`` with device draws: run twice from one checkpoint, and resumed from a
checkpoint, they repeat themselves bit for bit in fp32 and in bf16 rows, and torch's device generator is left alone -- each mode
in a fresh child process (tests/_reproducible_step_check.py) like tests/test_gpu_step_draws.py: a capture must precede the
network's first eager backward."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("mode", ["train2x_f32", "train2x_bf16", "resume"])
def test_steps_repeat_bit_for_bit(dev, mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_reproducible_step_check.py"), mode], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
