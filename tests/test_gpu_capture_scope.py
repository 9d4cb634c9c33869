"""hs_pose_amd/graph.py::capture_scope on its own -- the scaffold under GraphedStep, GraphedTrainStep, GraphedInference and
GraphedNetwork -- with no network built: the "module" is a BatchNorm1d(4) in train mode over a static (8, 4) input, the body that
forward plus one in-place add into a static output.  What the runners' tests do not isolate: how often and where the body runs,
the timer, the BatchNorm and sampler roll-back (also when a warm-up call raises), the capture stream, the shared pool."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

WARMUP = 3


class _Boom(Exception):
    pass


class _Rig:
    """the module, its static buffers, a sampler and a body that notes what it sees on every call"""

    def __init__(self, dev, raise_at=None):
        from hs_pose_amd import pc_sample
        g = torch.Generator().manual_seed(4)
        self.bn = torch.nn.BatchNorm1d(4).to(dev).train()
        with torch.no_grad():                                   # non-trivial statistics and affine terms
            self.bn.running_mean.copy_(torch.randn(4, generator=g))
            self.bn.running_var.copy_(torch.rand(4, generator=g) + 0.5)
            self.bn.num_batches_tracked.fill_(17)
            self.bn.weight.copy_(torch.rand(4, generator=g) + 0.5)
            self.bn.bias.copy_(torch.randn(4, generator=g))
        self.x = torch.randn(8, 4, generator=g).to(dev)
        self.out = torch.zeros(8, 4, device=dev)
        self.sampler = pc_sample.DeviceSampler(1234, dev)
        self.sampler.advance()                                  # (a key on the device that is not the initial zeros)
        self.raise_at, self.seen = raise_at, []

    def body(self):
        from hs_pose_amd import ops
        if len(self.seen) == self.raise_at:                     # host control flow only: before any GPU work of this call
            raise self.boom
        capturing = torch.cuda.is_current_stream_capturing()
        self.seen.append((capturing, ops._timer, torch.cuda.current_stream()))
        if not capturing:                                       # (as pc_sample.draw_scope: a captured body never advances)
            self.sampler.advance()
        with torch.no_grad():
            self.out.add_(self.bn(self.x))

    def state(self):
        torch.cuda.synchronize()
        return ([b.clone() for b in (self.bn.running_mean, self.bn.running_var, self.bn.num_batches_tracked)],
                self.sampler.get_state(), self.sampler.key.clone())

    def assert_state(self, want):
        torch.cuda.synchronize()
        bufs, state, key = self.state()
        for a, b in zip(bufs, want[0]):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert state == want[1] and torch.equal(key, want[2])


@pytest.fixture()
def timer():
    from hs_pose_amd import ops
    t = ops.KernelTimer()
    prev = ops.set_timer(t)
    yield t
    ops.set_timer(prev)


@pytest.mark.parametrize("on_warmup_stream", [False, True])
def test_scope_runs_warms_captures_and_restores(dev, timer, on_warmup_stream):
    from hs_pose_amd import ops
    from hs_pose_amd.graph import capture_scope
    rig = _Rig(dev)
    before = rig.state()
    with capture_scope(rig.bn, rig.sampler) as cap:
        cap.warm_up(rig.body, WARMUP)
        graph = cap.capture(rig.body, on_warmup_stream=on_warmup_stream)
    # the body ran warmup + 1 times: eagerly, then once under capture; never with a timer installed
    assert [c for c, _, _ in rig.seen] == [False] * WARMUP + [True]
    assert all(t is None for _, t, _ in rig.seen)
    assert ops._timer is timer
    streams = [s for _, _, s in rig.seen]
    assert all(s == streams[0] for s in streams[:WARMUP]) and streams[0] != torch.cuda.current_stream()
    if on_warmup_stream:
        assert streams[WARMUP] == streams[0]
    # train-mode forwards moved the statistics and advanced the sampler; both are back, bit for bit
    rig.assert_state(before)
    # a replay on new data == the eager body on that data
    twin = copy.deepcopy(rig.bn)
    x_new = torch.randn(8, 4, generator=torch.Generator().manual_seed(9)).to(dev)
    rig.x.copy_(x_new)
    rig.out.zero_()
    graph.replay()
    with torch.no_grad():
        want = torch.zeros(8, 4, device=dev).add_(twin(x_new))
    torch.cuda.synchronize()
    assert torch.equal(rig.out, want)
    for a, b in zip(rig.bn.buffers(), twin.buffers()):
        assert torch.equal(a, b)


def test_two_captures_share_a_pool(dev):
    from hs_pose_amd.graph import capture_scope
    rig = _Rig(dev)
    other = torch.zeros(8, 4, device=dev)

    def second():
        other.add_(rig.out)
    with capture_scope(rig.bn) as cap:
        cap.warm_up(lambda: (rig.body(), second()))
        first = cap.capture(rig.body)
        between = len(rig.seen)                                 # Python runs between the two captures of one scope
        graph2 = cap.capture(second, share_pool=first)
    assert between == 2 and first.pool() == graph2.pool()
    rig.out.zero_()
    other.zero_()
    first.replay()
    graph2.replay()
    torch.cuda.synchronize()
    assert torch.equal(other, rig.out) and bool(rig.out.abs().max() > 0)


def test_raising_warmup_restores_and_propagates(dev, timer):
    """the body raises a plain Python exception at the head of its second warm-up call (never inside a capture)"""
    from hs_pose_amd import ops
    from hs_pose_amd.graph import capture_scope
    rig = _Rig(dev, raise_at=1)
    rig.boom = _Boom("second warm-up call")
    before = rig.state()
    with pytest.raises(_Boom) as got:
        with capture_scope(rig.bn, rig.sampler) as cap:
            cap.warm_up(rig.body, WARMUP)
            cap.capture(rig.body)
    assert got.value is rig.boom
    assert [c for c, _, _ in rig.seen] == [False]               # one warm-up call ran, nothing was captured
    assert ops._timer is timer
    rig.assert_state(before)
    assert not torch.cuda.is_current_stream_capturing()
