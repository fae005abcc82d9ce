"""Differentiable neighbour observations captured into a HIP graph: the forward launch and the backward launch of _ops.neighbors_grad in ONE
torch.cuda.CUDAGraph at B = 2, E = 65 (the forward's rounds path), warmed up eagerly first.  Everything runs on the single capture stream -- the
leaves are made on it, autograd's backward runs its nodes on the stream their forward ran on -- so the capture is one chain of kernel nodes with no
parallel branches; the streams seen inside forward and backward are asserted to be that one.  Two replays, the inputs changed between them, equal
the eager runs bit for bit."""
import pytest
import torch

import neighbors_grad_model as gm
import neighbors_model as nm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_a_captured_forward_and_backward_replays_the_eager_bits():
    from torchdrivesim_amd import _ops
    seed, B, A, E, K, reach = gm.CASES['E65']
    t = {key: torch.from_numpy(v).to(DEV) for key, v in nm.random_scenes(seed, B, A, E).items()}
    assert t['boxes'].shape == (2, 65, 5)
    g = torch.randn((2, A, K, 8), generator=torch.Generator().manual_seed(65)).to(DEV)
    # the second set of inputs: everybody somewhere else and a little faster, another incoming gradient
    moved = {key: t[key].clone() for key in ('boxes', 'sc', 'speed')}
    moved['boxes'][..., 0] *= 0.9
    moved['boxes'][..., 1] += 0.25
    moved['speed'] *= 1.1
    inputs = [dict(t, g=g), dict(t, **moved, g=-2.0 * g)]
    static = {key: inputs[0][key].clone() for key in ('boxes', 'sc', 'speed', 'g')}
    seen = []

    def fwd_bwd(x):
        leaves = [x[key].detach().requires_grad_(True) for key in ('boxes', 'sc', 'speed')]
        features, index = _ops.neighbors_grad(*leaves, t['present'], A, K, reach)
        seen.append(torch.cuda.current_stream())
        features.register_hook(lambda grad: seen.append(torch.cuda.current_stream()))
        grads = torch.autograd.grad([features], leaves, [x['g']])
        return (features.detach(), index) + grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    del seen[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capture_stream = torch.cuda.current_stream()
        got = fwd_bwd(static)
    assert len(seen) == 2 and all(q == capture_stream for q in seen), 'forward and backward ran on the one capture stream'
    indices = []
    for x in inputs:
        want = fwd_bwd(x)
        for key in static:
            static[key].copy_(x[key])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
        for a, b in zip(got[2:], want[2:]):
            assert torch.equal(a, b)
        assert all(float(q.abs().max()) > 0 for q in want[2:]) and int((want[1] >= 0).sum()) >= 200
        indices.append(want[1].clone())
    assert not torch.equal(inputs[0]['boxes'], inputs[1]['boxes']) and not torch.equal(indices[0], indices[1]), 'the replays chose other neighbours'
