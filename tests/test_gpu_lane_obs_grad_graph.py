"""Differentiable lane observations captured into a HIP graph: the forward launch and the backward launch of _ops.lane_observations_grad in ONE
torch.cuda.CUDAGraph, B = 3 scenes (chain, fork, ring of 70) x 4 agents, after a warm-up call has built the lane tables (allocations and copies,
which a capture cannot hold) and run both launches eagerly.  Everything runs on the single capture stream -- the leaves are made on it,
autograd's backward runs its nodes on the stream their forward ran on -- so the capture is one chain of kernel nodes with no parallel branches;
the streams seen inside forward and backward are asserted to be that one.  Two replays, the inputs changed between them, equal the eager runs bit
for bit."""
import numpy as np
import pytest
import torch

import lane_obs_cases as cases
from test_gpu_lane_obs import make_sim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K, P, SPACING, REACH = 6, 13, 4.0, 100.0


def test_a_captured_forward_and_backward_replays_the_eager_bits():
    from torchdrivesim_amd import _ops
    maps = [cases.chain(), cases.fork(), cases.ring()]
    rng = np.random.default_rng(13)
    states = np.zeros((3, 4, 4), np.float32)
    for b, m in enumerate(maps):
        states[b, :, :3] = cases.poses(rng, m, 6)[2:]
    sim = make_sim(maps, states)
    lane_set = sim._lane_tables(torch.device(DEV))                  # built here, outside any capture
    present = sim.get_present_mask()
    xy, sc = sim.get_state()[..., :2].contiguous(), sim._heading_sc().detach()[:, :4].contiguous()
    gf = torch.randn((3, 4, K, 8), generator=torch.Generator().manual_seed(1)).to(DEV)
    gp = torch.randn((3, 4, K, P, 2), generator=torch.Generator().manual_seed(2)).to(DEV)
    # the second set of inputs: everybody a few metres on and turned, other incoming gradients
    turn = torch.tensor(0.4)
    moved_sc = torch.stack([sc[..., 0] * torch.cos(turn) + sc[..., 1] * torch.sin(turn), sc[..., 1] * torch.cos(turn) - sc[..., 0] * torch.sin(turn)], -1)
    inputs = [dict(xy=xy, sc=sc, gf=gf, gp=gp), dict(xy=xy + torch.tensor([3.0, -1.5], device=DEV), sc=moved_sc.contiguous(), gf=-2.0 * gf, gp=0.5 * gp)]
    static = {key: v.clone() for key, v in inputs[0].items()}
    seen = []

    def fwd_bwd(x):
        leaves = [x[key].detach().requires_grad_(True) for key in ('xy', 'sc')]
        features, points, n_valid, index = _ops.lane_observations_grad(lane_set, *leaves, present, K, P, SPACING, REACH)
        seen.append(torch.cuda.current_stream())
        features.register_hook(lambda grad: seen.append(torch.cuda.current_stream()))
        grads = torch.autograd.grad([features, points], leaves, [x['gf'], x['gp']])
        return (features.detach(), points.detach(), n_valid, index) + grads

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
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert all(float(q.abs().max()) > 0 for q in want[4:]) and int((want[3] >= 0).sum()) >= 30 and int(want[2].sum()) >= 100
        indices.append((want[3].clone(), want[2].clone()))
    assert not torch.equal(indices[0][0], indices[1][0]) or not torch.equal(indices[0][1], indices[1][1]), 'the replays chose other lanes or points'
