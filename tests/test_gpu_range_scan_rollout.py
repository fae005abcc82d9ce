"""The closed loop the differentiable range scans exist for: a vector policy in a ROLLOUT through the Simulator on the device.  T = 3 steps of a
KinematicBicycle, 2 scenes x 6 agents on the Town01 crop; in every step the agents scan 16 rays over 30 m
(compute_range_scan(differentiable=True)), act by  action_t = scale * tanh([road_t, agents_t] / max_range @ W)  with a fixed seeded W that
requires grad, and step.  The loss is a weighted sum of the ranges of all steps plus the final positions; ONE backward at the end.  The gradients
to state0 and W are held to the float64 torch model of the same chain (backward_models.bicycle_step_model,
range_scan_grad_model.ranges_given_choices), fed the device's witness of every step (_ops.range_scan_witness on the same inputs), at the project's
bar:
    |device - float64 model| <= 4 x the largest |float32 model - float64 model| per tensor
-- computed here from the model alone and printed beside the device's figure (run with -s) before anything is asserted.  Before that: through the
Simulator the flag gives today's bits, nothing is recorded without it or under no_grad, and the gradient to a state leaf, psi included, equals the
float64 chain model.  Last: step + scan + backward captured into one graph replays the eager bits."""
import numpy as np
import pytest
import torch

import backward_models as bm
import range_scan_grad_model as gm
import rollout_model as rom
from test_gpu_rollout import dev, make_sim

pytestmark = pytest.mark.gpu
FACTOR = 4.0
B, A, T, R, RANGE, GAP = 2, 6, 3, 16, 30.0, 0.02
SCALE = (1.0, 0.3)


def inputs():
    """a cluster of six within +-9 m of a vertex of the crop per scene, at 2 .. 10 m/s"""
    gen = np.random.default_rng(55)
    verts = rom.crop()[0]
    xy = verts[gen.integers(0, len(verts), B)][:, None, :] + gen.uniform(-9.0, 9.0, (B, A, 2))
    state0 = np.concatenate([xy, gen.uniform(-np.pi, np.pi, (B, A, 1)), gen.uniform(2.0, 10.0, (B, A, 1))], -1).astype(np.float32)
    size = np.stack([gen.uniform(4.0, 5.0, (B, A)), gen.uniform(1.8, 2.2, (B, A))], -1).astype(np.float32)
    return dict(state0=state0, size=size, lr=gen.uniform(1.0, 2.0, (B, A)).astype(np.float32), present=np.ones((B, A), bool),
                W=(0.3 * gen.standard_normal((2 * R, 2))).astype(np.float32), wa=gen.standard_normal((T, B, A, R)).astype(np.float32),
                wr=gen.standard_normal((T, B, A, R)).astype(np.float32), wp=gen.standard_normal((B, A, 2)).astype(np.float32))


def witness_of(sim):
    """the kernel's choices for the scan the simulator would compute now, and the constants of the rays that are not live"""
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import _static_maps_for
    with torch.no_grad():
        st = sim.get_all_agent_state().detach()
        boxes = torch.cat([st[..., :2], sim.get_all_agent_size().detach(), st[..., 2:3]], -1)
        ray_sc = _ops.heading_sc(sim.get_state()[..., 2].detach().unsqueeze(-1) + sim.range_scan_angles(R, device=st.device))
        smap = _static_maps_for(sim.road_mesh, st.device)
        choice, edge = _ops.range_scan_witness(smap, boxes, sim._heading_sc().detach(), sim.get_all_agent_present_mask(), ray_sc, A, RANGE, GAP)
    return choice.cpu().numpy(), edge.cpu().numpy()


def model_scan(s, size, off, choice, edge, const_a, const_r, dtype):
    """the scan of state s (B, A, 4) in `dtype` given the device's choices: the differentiated expression where a ray is live, the device's own
    value (0 or max_range, a constant) elsewhere"""
    boxes = torch.cat([s[..., :2], size, s[..., 2:3]], -1)
    sc = torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1)
    ang = s[..., 2, None] + off
    ray_sc = torch.stack([torch.sin(ang), torch.cos(ang)], -1)
    ta, la, tr, lr = gm.ranges_given_choices(boxes, sc, ray_sc, torch.from_numpy(choice.astype(np.int64)), torch.from_numpy(edge.astype(np.float64)))
    return torch.where(la, ta, const_a.to(dtype)), torch.where(lr, tr, const_r.to(dtype)), la, lr


def device_rollout(inp, differentiable):
    leaves = dict(state0=dev(inp['state0']).requires_grad_(True), lr=dev(inp['lr']), size=dev(inp['size']))
    W = dev(inp['W']).requires_grad_(True)
    sim = make_sim(inp, leaves, {})
    scale, wa, wr, wp = dev(np.array(SCALE, np.float32)), dev(inp['wa']), dev(inp['wr']), dev(inp['wp'])
    loss, steps = 0.0, []
    for t in range(T):
        choice, edge = witness_of(sim)
        scan = sim.compute_range_scan(n_rays=R, max_range=RANGE, gap_tolerance=GAP, differentiable=differentiable)
        assert scan.agents.requires_grad == differentiable and scan.road.requires_grad == differentiable and not scan.hit.requires_grad
        steps.append(dict(choice=choice, edge=edge, agents=scan.agents.detach().cpu(), road=scan.road.detach().cpu(), hit=scan.hit.cpu()))
        loss = loss + (scan.agents * wa[t]).sum() + (scan.road * wr[t]).sum()
        sim.step(scale * torch.tanh(torch.cat([scan.road, scan.agents], -1) / RANGE @ W))
    loss = loss + (sim.get_state()[..., :2] * wp).sum()
    loss.backward()
    torch.cuda.synchronize()
    return dict(state0=leaves['state0'].grad.double().cpu(), W=W.grad.double().cpu(), loss=float(loss.detach()), final=sim.get_state().detach().double().cpu()), steps


def model_rollout(inp, steps, dtype):
    """the same chain by torch autograd in `dtype`, the choices of every ray of every step given"""
    from torchdrivesim_amd.simulator import Simulator
    t_ = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    s = t_(inp['state0']).requires_grad_(True)
    W = t_(inp['W']).requires_grad_(True)
    size, lr, scale, wa, wr, wp = t_(inp['size']), t_(inp['lr']), t_(np.array(SCALE, np.float32)), t_(inp['wa']), t_(inp['wr']), t_(inp['wp'])
    off = Simulator.range_scan_angles(R).to(dtype)
    leaves, loss, live = (s, W), 0.0, 0
    for t in range(T):
        agents, road, la, lr_ = model_scan(s, size, off, steps[t]['choice'], steps[t]['edge'], steps[t]['agents'], steps[t]['road'], dtype)
        live += int(la.sum()) + int(lr_.sum())
        loss = loss + (agents * wa[t]).sum() + (road * wr[t]).sum()
        s = bm.bicycle_step_model(s, scale * torch.tanh(torch.cat([road, agents], -1) / RANGE @ W), lr)
    loss = loss + (s[..., :2] * wp).sum()
    g = torch.autograd.grad(loss, leaves)
    return dict(state0=g[0].double(), W=g[1].double(), loss=float(loss.detach()), final=s.detach().double(), live=live)


def bar(label, got, m64, m32, keys):
    failures = []
    for key in keys:
        diff, yard, scale = float((got[key] - m64[key]).abs().max()), float((m32[key] - m64[key]).abs().max()), float(m64[key].abs().max())
        print(f'{label} {key}: device against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}')
        if not diff <= FACTOR * yard:
            failures.append(f'{key}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not bool(torch.isfinite(got[key]).all()):
            failures.append(f'{key}: not finite')
    assert not failures, '\n'.join(failures)


def test_through_the_simulator():
    """one scan: today's bits, no graph without the flag or under no_grad, and the gradient to the state leaf -- x, y and psi (through the agent's
    [sin, cos] and its rays') -- against the float64 chain model fed the witness"""
    inp = inputs()
    leaves = dict(state0=dev(inp['state0']), lr=dev(inp['lr']), size=dev(inp['size']))
    sim = make_sim(inp, leaves, {})
    kw = dict(n_rays=R, max_range=RANGE, gap_tolerance=GAP)
    plain = sim.compute_range_scan(**kw)
    assert plain.agents.grad_fn is None and not plain.road.requires_grad
    quiet = sim.compute_range_scan(differentiable=True, **kw)                                # nothing requires grad
    assert quiet.agents.grad_fn is None and quiet.road.grad_fn is None and torch.equal(quiet.road, plain.road)
    leaf = dev(inp['state0']).requires_grad_(True)
    sim.kinematic_model.set_state(leaf)
    for off in (sim.compute_range_scan(**kw), sim.compute_range_scan(differentiable=False, **kw)):
        assert off.agents.grad_fn is None and off.road.grad_fn is None and not off.agents.requires_grad
    with torch.no_grad():
        off = sim.compute_range_scan(differentiable=True, **kw)
    assert off.agents.grad_fn is None and off.road.grad_fn is None and torch.equal(off.agents, plain.agents)
    choice, edge = witness_of(sim)
    scan = sim.compute_range_scan(differentiable=True, **kw)
    assert scan.agents.requires_grad and scan.road.requires_grad and not scan.hit.requires_grad and scan.hit.grad_fn is None
    for a, b in ((scan.agents, plain.agents), (scan.road, plain.road), (scan.hit, plain.hit)):
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32)), 'the forward bits are today\'s'
    gen = torch.Generator().manual_seed(5)
    ga, gr = torch.randn(scan.agents.shape, generator=gen), torch.randn(scan.road.shape, generator=gen)
    torch.autograd.backward([scan.agents, scan.road], [ga.to(leaf.device), gr.to(leaf.device)])
    got = dict(state=leaf.grad.double().cpu())
    from torchdrivesim_amd.simulator import Simulator
    ref = {}
    for dtype in (torch.float64, torch.float32):
        s = torch.from_numpy(inp['state0']).to(dtype).requires_grad_(True)
        agents, road, la, lr = model_scan(s, torch.from_numpy(inp['size']).to(dtype), Simulator.range_scan_angles(R).to(dtype), choice, edge,
                                          plain.agents.cpu(), plain.road.cpu(), dtype)
        ref[dtype] = dict(state=torch.autograd.grad((agents * ga.to(dtype)).sum() + (road * gr.to(dtype)).sum(), s)[0].double())
    print(f'Simulator: live rays: agents {int(la.sum())}, road {int(lr.sum())} of {la.numel()}')
    assert int(la.sum()) >= 10 and int(lr.sum()) >= 60
    assert torch.equal(torch.from_numpy(choice[..., 0])[plain.hit.cpu() >= 0], plain.hit.cpu()[plain.hit.cpu() >= 0])
    bar('Simulator g_state', got, ref[torch.float64], ref[torch.float32], ('state',))
    assert all(float(got['state'][..., col].abs().max()) > 0 for col in range(3)) and not got['state'][..., 3].any(), 'x, y, psi; the speed is not read'


def test_a_vector_policy_rollout_against_the_float64_model():
    inp = inputs()
    got, steps = device_rollout(inp, True)
    m64, m32 = model_rollout(inp, steps, torch.float64), model_rollout(inp, steps, torch.float32)
    assert m64['live'] >= T * 60, 'most road rays end on an edge within reach'
    rel = bm.step_forward_rel(inp['state0'].astype(np.float64), got['final'].numpy(), m64['final'].numpy())
    print(f'range-scan rollout: final state rel {rel:.3g} over {T} steps (bar 1e-5 a step), loss {got["loss"]:.6g} against {m64["loss"]:.6g}, '
          f'live rays {m64["live"]} of {2 * T * B * A * R}')
    bar('range-scan rollout', got, m64, m32, ('state0', 'W'))
    assert rel <= T * 1e-5
    assert int((got['state0'] != 0).sum()) * 2 >= got['state0'].numel() and int((got['W'] != 0).sum()) * 2 >= got['W'].numel()
    # the path state -> observation -> action: cut, as before the observation had a gradient, state0 gets another gradient
    cut, cut_steps = device_rollout(inp, False)
    assert all(torch.equal(x['road'], y['road']) and torch.equal(x['agents'], y['agents']) for x, y in zip(steps, cut_steps)) and cut['loss'] == got['loss']
    gap = float((cut['state0'] - got['state0']).abs().max())
    print(f'range-scan rollout: without the path through the observation g_state0 differs by {gap:.3g} of {float(got["state0"].abs().max()):.3g}')
    assert gap > 100 * FACTOR * float((m32['state0'] - m64['state0']).abs().max()) and gap > 0.01 * float(got['state0'].abs().max())


def test_a_captured_step_scan_and_backward_replays_the_eager_bits():
    """everything on the one capture stream, warmed up eagerly first (the device map exists before the capture)"""
    inp = inputs()
    leaves = dict(state0=dev(inp['state0']), lr=dev(inp['lr']), size=dev(inp['size']))
    sim = make_sim(inp, leaves, {})
    gen = torch.Generator().manual_seed(8)
    sets = [dict(state=dev(inp['state0']) + shift, action=(torch.rand((B, A, 2), generator=gen) * 2 - 1).to(shift.device) * dev(np.array(SCALE, np.float32)),
                 ga=torch.randn((B, A, R), generator=gen).to(shift.device), gr=torch.randn((B, A, R), generator=gen).to(shift.device))
            for shift in (dev(np.zeros(4, np.float32)), dev(np.array([0.4, -0.3, 0.05, 0.5], np.float32)))]
    static = {key: v.clone() for key, v in sets[0].items()}

    def run(x):
        leaf = x['state'].detach().requires_grad_(True)
        sim.kinematic_model.set_state(leaf)
        sim.step(x['action'])
        scan = sim.compute_range_scan(n_rays=R, max_range=RANGE, gap_tolerance=GAP, differentiable=True)
        grad, = torch.autograd.grad([scan.agents, scan.road], [leaf], [x['ga'], x['gr']])
        return scan.agents.detach(), scan.road.detach(), scan.hit, grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run(static)
    for x in sets:
        want = [v.clone() for v in run(x)]
        for key in static:
            static[key].copy_(x[key])
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert float(want[3].abs().max()) > 0 and bool((want[1] < RANGE).any())
