"""The closed loop the differentiable lane observations exist for: a lane-keeping vector policy in a ROLLOUT through the Simulator on the device.
T = 3 steps of a KinematicBicycle, 2 scenes (chain(), fork()) x 4 agents; in every step the agents observe their lanes
(compute_lanes(k=3, n_points=4, differentiable=True)), act by  action_t = scale * tanh([lateral, sin_rel, point 0, point 1 of slot 0] @ W)  with a
fixed seeded W that requires grad, and step.  The loss is a weighted sum of the features and points of all steps plus the final positions; ONE
backward at the end.  The gradients to state0 and W are held to the float64 torch model of the same chain (backward_models.bicycle_step_model,
lane_obs_grad_model.observations), which makes its own discrete choices from its own states, at the project's bar:
    |device - float64 model| <= 4 x the largest |float32 model - float64 model| per tensor
-- computed here from the model alone and printed beside the device's figure (run with -s) before anything is asserted.  The poses keep at least
0.5 m from every segment end, and index and n_valid of every step must equal the model's: a crossed kink fails loudly instead of widening the
error.  And the path through the observation matters: with differentiable=False, which is what the code computed before, the gradient to state0
is another one."""
import numpy as np
import pytest
import torch

import backward_models as bm
import lane_obs_cases as cases
import lane_obs_grad_model as gm
import lane_obs_model as lom
from test_gpu_lane_obs import make_sim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
B, A, T, K, P, SPACING, REACH = 2, 4, 3, 3, 4, 4.0, 30.0
SCALE = (1.0, 0.3)
LR = 1.9                    # what test_gpu_lane_obs.make_sim gives every agent
LATERAL, SIN_REL = 6, 2


def inputs():
    """four agents a scene beside straight lanelets -- on the fork all four beside lanelet 0, before the branch, two on either side of it --, at
    least 1.3 m after a centre-line point and 2.5 m before the next (the lines have a point every 5 or 2.5 m; three steps at 2 .. 4 m/s are
    1.2 m at most), 0.4 .. 1 m off the line, headings within 0.2 rad of the lane's.  The feet on the other lanelets are clamped to their ends"""
    gen = np.random.default_rng(8)
    x = np.array([[1.3, 6.3, 13.1, 21.3], [1.3, 6.3, 2.2, 7.2]])
    side = np.array([[-1.0, -1.0, -1.0, -1.0], [-1.0, -1.0, 1.0, 1.0]])
    state0 = np.stack([x, side * gen.uniform(0.4, 1.0, (B, A)), gen.uniform(-0.2, 0.2, (B, A)), gen.uniform(2.0, 4.0, (B, A))], -1).astype(np.float32)
    return dict(state0=state0, W=(0.3 * gen.standard_normal((6, 2))).astype(np.float32), wf=gen.standard_normal((T, B, A, K, 8)).astype(np.float32),
                wq=gen.standard_normal((T, B, A, K, P, 2)).astype(np.float32), wp=gen.standard_normal((B, A, 2)).astype(np.float32))


def policy_inputs(features, points):
    return torch.cat([features[:, :, 0, LATERAL:LATERAL + 1], features[:, :, 0, SIN_REL:SIN_REL + 1], points[:, :, 0, :2].flatten(-2)], -1)


def device_rollout(maps, inp, differentiable):
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    state0, W = dev(inp['state0']).requires_grad_(True), dev(inp['W']).requires_grad_(True)
    sim = make_sim(maps, inp['state0'])
    sim.kinematic_model.set_state(state0)
    scale, wf, wq, wp = dev(np.array(SCALE, np.float32)), dev(inp['wf']), dev(inp['wq']), dev(inp['wp'])
    loss, seen = 0.0, []
    for t in range(T):
        obs = sim.compute_lanes(k=K, n_points=P, spacing=SPACING, max_distance=REACH, differentiable=differentiable)
        assert obs.features.requires_grad == differentiable and obs.points.requires_grad == differentiable and not obs.index.requires_grad
        seen.append((obs.index.cpu().numpy(), obs.n_valid.cpu().numpy()))
        loss = loss + (obs.features * wf[t]).sum() + (obs.points * wq[t]).sum()
        sim.step(scale * torch.tanh(policy_inputs(obs.features, obs.points) @ W))
    loss = loss + (sim.get_state()[..., :2] * wp).sum()
    loss.backward()
    torch.cuda.synchronize()
    return dict(state0=state0.grad.double().cpu(), W=W.grad.double().cpu(), loss=float(loss.detach()), final=sim.get_state().detach().double().cpu()), seen


def model_rollout(lanes, inp, dtype):
    """the same chain by torch autograd in `dtype`; the discrete choices of every step are those of the forward model at the model's own poses"""
    t_ = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    s = t_(inp['state0']).requires_grad_(True)
    W = t_(inp['W']).requires_grad_(True)
    leaves = (s, W)
    lr, scale, wf, wq, wp = torch.full((B, A), LR, dtype=dtype), t_(np.array(SCALE, np.float32)), t_(inp['wf']), t_(inp['wq']), t_(inp['wp'])
    loss, seen = 0.0, []
    for t in range(T):
        X = torch.cat([s[..., :2], torch.sin(s[..., 2:3]), torch.cos(s[..., 2:3])], -1)
        pose = X.detach().numpy().astype(np.float32)
        _, _, n_valid, index = lom.observe_batch(lanes, pose[..., :2], pose[..., 2:], np.ones((B, A), bool), K, P, SPACING, REACH)
        seen.append((index, n_valid))
        filled, valid, S, Q = gm.constants(lanes, pose[..., :2], pose[..., 2:], index, P, SPACING)
        assert np.array_equal(filled, index >= 0) and np.array_equal(valid.sum(-1), n_valid)
        feats, pts, at_slots, at_points = gm.observations(X, S, Q, SPACING)
        features = torch.zeros((B, A, K, 8), dtype=dtype).index_put(tuple(torch.as_tensor(v) for v in at_slots), feats)
        points = torch.zeros((B, A, K, P, 2), dtype=dtype).index_put(tuple(torch.as_tensor(v) for v in at_points), pts)
        loss = loss + (features * wf[t]).sum() + (points * wq[t]).sum()
        s = bm.bicycle_step_model(s, scale * torch.tanh(policy_inputs(features, points) @ W), lr)
    loss = loss + (s[..., :2] * wp).sum()
    g = torch.autograd.grad(loss, leaves)
    return dict(state0=g[0].double(), W=g[1].double(), loss=float(loss.detach()), final=s.detach().double()), seen


def test_a_lane_keeping_rollout_against_the_float64_model():
    maps = [cases.chain(), cases.fork()]
    lanes = [lom.Lanes(m) for m in maps]
    inp = inputs()
    got, seen = device_rollout(maps, inp, True)
    (m64, seen64), (m32, seen32) = model_rollout(lanes, inp, torch.float64), model_rollout(lanes, inp, torch.float32)
    for t in range(T):
        for model in (seen64, seen32):
            assert np.array_equal(seen[t][0], model[t][0]) and np.array_equal(seen[t][1], model[t][1]), f'step {t}: index or n_valid is not the model\'s'
        assert (seen[t][0] >= 0).all() and (seen[t][1] >= 1).all() and (seen[t][1] < P).any(), 'every slot is filled; some polylines end early'
    rel = bm.step_forward_rel(inp['state0'].astype(np.float64), got['final'].numpy(), m64['final'].numpy())
    print(f'lane rollout: final state rel {rel:.3g} over {T} steps (bar 1e-5 a step), loss {got["loss"]:.6g} against {m64["loss"]:.6g}')
    failures = []
    for key in ('state0', 'W'):
        diff, yard, scale = float((got[key] - m64[key]).abs().max()), float((m32[key] - m64[key]).abs().max()), float(m64[key].abs().max())
        print(f'lane rollout {key}: device against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}')
        if not diff <= FACTOR * yard:
            failures.append(f'{key}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not bool(torch.isfinite(got[key]).all()):
            failures.append(f'{key}: not finite')
    assert not failures, '\n'.join(failures)
    assert rel <= T * 1e-5
    assert int((got['state0'][..., :3] != 0).sum()) == B * A * 3 and int((got['W'] != 0).sum()) == got['W'].numel()
    # the path state -> observation -> action: cut, as before the observation had a gradient, state0 gets another gradient
    cut, cut_seen = device_rollout(maps, inp, False)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(seen, cut_seen)) and cut['loss'] == got['loss'], 'the forward is the same'
    gap = float((cut['state0'] - got['state0']).abs().max())
    print(f'lane rollout: without the path through the observation g_state0 differs by {gap:.3g} of {float(got["state0"].abs().max()):.3g}')
    assert gap > 100 * FACTOR * float((m32['state0'] - m64['state0']).abs().max()) and gap > 0.01 * float(got['state0'].abs().max())
