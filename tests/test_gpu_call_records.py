"""GPU: the libhsp calls behind the public ops, held to a recording.

tests/golden/call_records.json was written by tools/record_op_calls.py on the commit BEFORE ops.py's marshalling moved into one raw
wrapper per entry-point family (41652d2).  Every case is run again here: the ordered (entry point, key, abytes, aflops) list that
``ops.KernelTimer`` sees must be the recorded one -- the same calls in the same order with the same roofline figures -- and the sha256
of every output and gradient must match, except the gradients of the two backwards that add in arrival order (the default pooling
backward with a per-query gradient, ``hsp_gather_rows_bwd``), whose values the reference tests hold."""
import json
import os

import pytest

from tools import record_op_calls as rec

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_records.json")

# every entry point whose marshalling has one wrapper now: a case that silently took another route leaves its name out
REQUIRED = [
    "hsp_gather_max_bwd", "hsp_gather_max_bwd_bf16", "hsp_gather_max_bwd_sel", "hsp_gather_max_bwd_sel_bf16",
    "hsp_gather_max_bwd_csr", "hsp_gather_max_bwd_csr_bf16", "hsp_gather_rows_bwd", "hsp_gather_rows_bwd_csr",
    "hsp_gather_rows_bwd_csr_bf16", "hsp_rf_surface_fwd", "hsp_rf_surface_fwd_bf16", "hsp_rf_surface_bwd", "hsp_rf_surface_bwd_bf16",
    "hsp_bn_relu_fwd", "hsp_bn_relu_fwd_bf16", "hsp_bn_relu_fwd_mixed", "hsp_bn_relu_fwd_partials", "hsp_bn_relu_fwd_partials_mixed",
    "hsp_bn_relu_bwd", "hsp_bn_relu_bwd_bf16", "hsp_bn_relu_bwd_mixed", "hsp_bn_relu_bwd2", "hsp_bn_relu_apply_bf16",
    "hsp_bn_relu_apply_mixed", "hsp_split_params_x3", "hsp_gemm_rows_f32", "hsp_gemm_rows_bf16", "hsp_gemm_wave_f32", "hsp_gemm_x3_f32",
    "hsp_gemm_x3_bn_f32", "hsp_gemm_x3_bias_bn_f32", "hsp_gemm_rows_acc_bf16",
    # the routes the cases were sized for: the two-launch per-cloud chain, its column sum as a rider of the pair launch
    "hsp_colsum_cloud_f32", "hsp_small_pair_f32", "hsp_wgrad_partial_pair_f32", "hsp_wgrad_partial_pair_colsum_f32",
]
# the key suffix of each form of the pooling / ORL backward (per query, per cloud kept rows, broadcast, accumulating, from counts)
REQUIRED_KEYS = [("hsp_gather_max_bwd", "bc"), ("hsp_gather_max_bwd", "bc+"), ("hsp_gather_max_bwd", "cnt+"), ("hsp_gather_max_bwd_sel", "pc"),
                 ("hsp_gather_max_bwd_bf16", "bc+"), ("hsp_gather_max_bwd_csr", "bc")]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_recording_reaches_every_family(recorded):
    assert sorted(recorded) == sorted(rec.CASES)
    names = rec.entry_points(recorded)
    assert not [n for n in REQUIRED if n not in names]
    calls = [c for r in recorded.values() for c in r["calls"]]
    assert not [(n, s) for n, s in REQUIRED_KEYS if not any(c[0] == n and c[1].endswith(s) for c in calls)]
    plain = [c for c in calls if c[0] in ("hsp_gather_max_bwd", "hsp_gather_max_bwd_bf16") and c[1][-1].isdigit()]
    assert plain                                               # (a gradient per query on the shared list: no suffix at all)


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_calls_and_bits_are_the_recorded_ones(dev, recorded, name):
    got, want = rec.run_case(name, dev), recorded[name]
    assert got["calls"] == want["calls"]
    assert got["outputs"] == want["outputs"]
    assert got["grads"] == want["grads"]
