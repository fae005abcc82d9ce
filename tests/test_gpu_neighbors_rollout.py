"""The closed loop the differentiable neighbour observations exist for: a vector policy in a ROLLOUT through the Simulator on the device.  T = 3
steps of a KinematicBicycle, 2 scenes x 6 agents on the Town01 crop; in every step the agents observe their three nearest neighbours
(compute_neighbors(k=3, differentiable=True)), act by  action_t = scale * tanh(features_t[:, :, :3].flatten(-2) @ W)  with a fixed seeded W that
requires grad, and step.  The loss is a weighted sum of the features of all steps plus the final positions; ONE backward at the end.  The gradients
to state0 and W are held to the float64 torch model of the same chain (backward_models.bicycle_step_model, neighbors_grad_model.features), fed the
device's index of every step, at the project's bar:
    |device - float64 model| <= 4 x the largest |float32 model - float64 model| per tensor
-- computed here from the model alone and printed beside the device's figure (run with -s) before anything is asserted.  And the path through the
observation matters: with differentiable=False, which is what the code computed before, the gradient to state0 is another one."""
import numpy as np
import pytest
import torch

import backward_models as bm
import neighbors_grad_model as gm
import rollout_model as rom
from test_gpu_rollout import dev, make_sim

pytestmark = pytest.mark.gpu
FACTOR = 4.0
B, A, T, K, REACH = 2, 6, 3, 3, 50.0
SCALE = (1.0, 0.3)


def inputs():
    """a cluster of six within +-12 m of a vertex of the crop per scene, at 2 .. 10 m/s; agent 5 of scene 1 stands 80 m away: nobody's neighbour,
    and its own row is empty"""
    gen = np.random.default_rng(66)
    verts = rom.crop()[0]
    xy = verts[gen.integers(0, len(verts), B)][:, None, :] + gen.uniform(-12.0, 12.0, (B, A, 2))
    xy[1, 5] += 80.0
    state0 = np.concatenate([xy, gen.uniform(-np.pi, np.pi, (B, A, 1)), gen.uniform(2.0, 10.0, (B, A, 1))], -1).astype(np.float32)
    size = np.stack([gen.uniform(4.0, 5.0, (B, A)), gen.uniform(1.8, 2.2, (B, A))], -1).astype(np.float32)
    return dict(state0=state0, size=size, lr=gen.uniform(1.0, 2.0, (B, A)).astype(np.float32), present=np.ones((B, A), bool),
                W=(0.05 * gen.standard_normal((K * 8, 2))).astype(np.float32), wf=gen.standard_normal((T, B, A, K, 8)).astype(np.float32),
                wp=gen.standard_normal((B, A, 2)).astype(np.float32))


def device_rollout(inp, differentiable):
    leaves = dict(state0=dev(inp['state0']).requires_grad_(True), lr=dev(inp['lr']), size=dev(inp['size']))
    W = dev(inp['W']).requires_grad_(True)
    sim = make_sim(inp, leaves, {})
    scale, wf, wp = dev(np.array(SCALE, np.float32)), dev(inp['wf']), dev(inp['wp'])
    loss, indices = 0.0, []
    for t in range(T):
        nb = sim.compute_neighbors(k=K, max_distance=REACH, differentiable=differentiable)
        assert nb.features.requires_grad == differentiable and not nb.index.requires_grad
        indices.append(nb.index.cpu().numpy())
        loss = loss + (nb.features * wf[t]).sum()
        sim.step(scale * torch.tanh(nb.features[:, :, :3].flatten(-2) @ W))
    loss = loss + (sim.get_state()[..., :2] * wp).sum()
    loss.backward()
    torch.cuda.synchronize()
    return dict(state0=leaves['state0'].grad.double().cpu(), W=W.grad.double().cpu(), loss=float(loss.detach()), final=sim.get_state().detach().double().cpu()), indices


def model_rollout(inp, indices, dtype):
    """the same chain by torch autograd in `dtype`, the entity of every slot of every step given"""
    t_ = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    s = t_(inp['state0']).requires_grad_(True)
    W = t_(inp['W']).requires_grad_(True)
    leaves = (s, W)
    size, lr, scale, wf, wp = t_(inp['size']), t_(inp['lr']), t_(np.array(SCALE, np.float32)), t_(inp['wf']), t_(inp['wp'])
    loss = 0.0
    for t in range(T):
        V = torch.cat([s[..., :2], size, torch.sin(s[..., 2:3]), torch.cos(s[..., 2:3]), s[..., 3:4]], -1)
        _, b, a, k, e = gm.filled_slots(indices[t], A)
        b, a, k, e = (torch.as_tensor(v) for v in (b, a, k, e))
        feat = torch.zeros((B, A, K, 8), dtype=dtype).index_put((b, a, k), gm.features(V, b, a, e))
        loss = loss + (feat * wf[t]).sum()
        s = bm.bicycle_step_model(s, scale * torch.tanh(feat[:, :, :3].flatten(-2) @ W), lr)
    loss = loss + (s[..., :2] * wp).sum()
    g = torch.autograd.grad(loss, leaves)
    return dict(state0=g[0].double(), W=g[1].double(), loss=float(loss.detach()), final=s.detach().double())


def test_a_vector_policy_rollout_against_the_float64_model():
    inp = inputs()
    got, indices = device_rollout(inp, True)
    filled = np.stack(indices) >= 0
    assert filled.sum() >= T * (B * A * K - 2 * K) and not filled[:, 1, 5].any() and filled[:, 0].all(), 'agent 5 of scene 1 sees nobody; scene 0 is full'
    m64, m32 = model_rollout(inp, indices, torch.float64), model_rollout(inp, indices, torch.float32)
    rel = bm.step_forward_rel(inp['state0'].astype(np.float64), got['final'].numpy(), m64['final'].numpy())
    print(f'neighbour rollout: final state rel {rel:.3g} over {T} steps (bar 1e-5 a step), loss {got["loss"]:.6g} against {m64["loss"]:.6g}')
    failures = []
    for key in ('state0', 'W'):
        diff, yard, scale = float((got[key] - m64[key]).abs().max()), float((m32[key] - m64[key]).abs().max()), float(m64[key].abs().max())
        print(f'neighbour rollout {key}: device against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}')
        if not diff <= FACTOR * yard:
            failures.append(f'{key}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not bool(torch.isfinite(got[key]).all()):
            failures.append(f'{key}: not finite')
    assert not failures, '\n'.join(failures)
    assert rel <= T * 1e-5
    assert int((got['state0'] != 0).sum()) * 2 >= got['state0'].numel() and int((got['W'] != 0).sum()) == got['W'].numel()
    # the path state -> observation -> action: cut, as before the observation had a gradient, state0 gets another gradient
    cut, cut_indices = device_rollout(inp, False)
    assert all(np.array_equal(x, y) for x, y in zip(indices, cut_indices)) and cut['loss'] == got['loss'], 'the forward is the same'
    gap = float((cut['state0'] - got['state0']).abs().max())
    print(f'neighbour rollout: without the path through the observation g_state0 differs by {gap:.3g} of {float(got["state0"].abs().max()):.3g}')
    assert gap > 100 * FACTOR * float((m32['state0'] - m64['state0']).abs().max()) and gap > 0.01 * float(got['state0'].abs().max())
