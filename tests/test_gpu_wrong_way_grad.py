"""The wrong-way loss's gradient to psi on the device (csrc/lanes.hip `tds_wrong_way_grad_f32`; _ops.wrong_way_grad;
infractions.lanelet_orientation_loss(differentiable=True)).

`out` must be tds_wrong_way_f32's own bits, the gradient reaches psi alone, and the derivative is accepted WITHOUT exclusions by this rule: for
every agent there is a lanelet among those the device itself lists for its position (_ops.lanelet_directions) whose float64 loss is within the
forward's existing 2e-6 of the kernel's loss AND whose float64 derivative is within the house bar -- 4 x the largest |float32 model - float64
model| over the tensor -- of the kernel's dloss_dpsi.  Two lanelets can tie at the minimum to 1e-5 with different derivatives, so a model that
picked its own minimum would need exclusions; "some lanelet attaining the minimum" needs none."""
import math

import numpy as np
import pytest
import torch

from test_lanelet2 import KAT_LEFT, KAT_RIGHT, _agents, town01  # noqa: F401  (town01: the module's fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64
FACTOR = 4.0
LOSS_TOLERANCE = 2e-6            # tests/test_lanelet2.py: the forward against the oracle
CASES = ((math.pi / 2, 1.0), (2.0, 0.25))
OFFSET = np.array([[0.5, -0.25], [-1.0, 2.0]], F32)


def models(dirs, psi, thr):
    """dirs (n, m) float64, psi (n,) float32 -> float64 loss (n, m), float64 derivative, float32-model derivative: -cos(delta) and -sin(delta)
    times [|delta| > thr], delta = normalize_angle(direction - psi); the float32 model rounds as the kernel's definition does (the direction to
    float32, the difference, normalize_angle and the sine in float32)"""
    d64 = np.remainder(dirs - psi.astype(F64)[:, None] + math.pi, 2 * math.pi) - math.pi
    over64 = np.abs(d64) > thr
    d32 = np.remainder((dirs.astype(F32) - psi[:, None]) + F32(math.pi), F32(2 * math.pi)) - F32(math.pi)
    over32 = np.abs(d32) > F32(thr)
    return -np.cos(d64) * over64, -np.sin(d64) * over64, (-np.sin(d32) * over32).astype(F64), -np.sin(d64), -np.sin(d32).astype(F64)


def run(maps, state, offset, thr, tol, present=None):
    """-> (plain loss, differentiable loss, dloss_dpsi, the gradient of sum(g * loss) to the state, g), numpy"""
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import lane_table_set, lanelet_orientation_loss
    st = torch.from_numpy(state).to(DEV)
    off = None if offset is None else torch.from_numpy(offset).to(DEV)
    lane_set = lane_table_set(maps, torch.device(DEV), tol)
    plain = lanelet_orientation_loss(maps, st, off, thr, tol, lane_set=lane_set)
    assert plain.grad_fn is None and not plain.requires_grad
    leaf = st.clone().requires_grad_(True)
    for quiet in (lanelet_orientation_loss(maps, leaf, off, thr, tol, lane_set=lane_set), lanelet_orientation_loss(maps, st, off, thr, tol, lane_set=lane_set,
                                                                                                                      differentiable=True)):
        assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet.view(torch.int32), plain.view(torch.int32))
    with torch.no_grad():
        quiet = lanelet_orientation_loss(maps, leaf, off, thr, tol, lane_set=lane_set, differentiable=True)
    assert quiet.grad_fn is None and not quiet.requires_grad
    out = lanelet_orientation_loss(maps, leaf, off, thr, tol, lane_set=lane_set, differentiable=True)
    pres = None if present is None else torch.from_numpy(present).to(DEV)
    if lane_set is None:                                  # no map at all: zeros, nothing to record
        assert out.grad_fn is None and not out.any()
        return plain.cpu().numpy(), out.cpu().numpy(), np.zeros(out.shape, F32), np.zeros(state.shape, F32), np.zeros(out.shape, F32)
    assert out.requires_grad and out.grad_fn is not None and out.dtype == torch.float32
    again, dpsi = _ops.wrong_way(lane_set, st, off, pres, thr, tol, want_dpsi=True)
    if present is None:
        assert torch.equal(again.view(torch.int32), plain.view(torch.int32)), 'the two entry points write the same bits'
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    torch.autograd.backward([out], [g])
    return plain.cpu().numpy(), out.detach().cpu().numpy(), dpsi.cpu().numpy(), leaf.grad.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize('thr,tol', CASES)
@pytest.mark.parametrize('with_offset', [False, True])
def test_town01_poses(town01, with_offset, thr, tol):
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import lane_table_set
    B, A = 2, 48
    state = _agents(town01, B, A, 3)
    offset = OFFSET if with_offset else None
    maps = [town01, town01]
    plain, out, dpsi, grad, g = run(maps, state, offset, thr, tol)
    assert np.array_equal(out.view(np.int32), plain.view(np.int32)), 'out is tds_wrong_way_f32\'s bits'
    # the gradient reaches psi only, and it is g * dloss_dpsi
    assert not grad[..., [0, 1, 3]].any() and np.array_equal(grad[..., 2], g * dpsi)
    # the lanelets the device lists for the positions the kernel used (float32 position plus float32 offset, widened)
    xy = state[..., :2] if offset is None else state[..., :2] + offset[:, None]
    lane_set = lane_table_set(maps, torch.device(DEV), tol)
    dirs, _, count, status = (t.cpu().numpy() for t in _ops.lanelet_directions(lane_set, None, torch.from_numpy(xy.reshape(-1, 2).astype(F64)).to(DEV), tol,
                                                                                  max_dirs=16))
    assert count.max() <= 16
    loss64, d64, d32, smooth64, smooth32 = models(dirs, state[..., 2].reshape(-1), thr)
    listed = np.arange(16)[None] < count[:, None]
    yard = float(np.abs(smooth64 - smooth32)[listed].max())          # the float32 model's own error of -sin(delta), over every listed lanelet
    forced = (count == 0) | (status != 0)
    kl, kd = out.reshape(-1).astype(F64), dpsi.reshape(-1).astype(F64)
    loss_gap = np.where(listed, np.abs(loss64 - kl[:, None]), np.inf)
    deriv_gap = np.where(listed, np.abs(d64 - kd[:, None]), np.inf)
    ok = (loss_gap <= LOSS_TOLERANCE) & (deriv_gap <= FACTOR * yard)
    best = np.where(loss_gap <= LOSS_TOLERANCE, deriv_gap, np.inf).min(-1)
    print(f'thr {thr:.4f} tol {tol} offset {with_offset}: {int((~forced).sum())} agents with lanelets ({int((count > 1).sum())} with several), kernel '
          f'derivative against the float64 derivative of a lanelet at the minimum {float(best[~forced].max()):.3g}, float32 model against float64 '
          f'{yard:.3g} (bound {FACTOR * yard:.3g}); {int((kd != 0).sum())} agents with a derivative, {int((kd == 0).sum())} without')
    assert ok[~forced].any(-1).all(), np.nonzero(~ok.any(-1) & ~forced)[0].tolist()
    assert not kl[forced].any() and not kd[forced].any(), 'no lanelet, an excluded tag or a failed find_direction: exactly 0'
    assert (kd != 0).sum() > 10 and (kd == 0).sum() > 10 and (kl > 0).sum() > 10
    assert not dpsi[0, :3].any() and not out[0, :3].any(), 'the strays and the NaN pose'
    assert not kd[kl == 0].any(), 'a loss of 0 is a winner inside the threshold: derivative 0'


def test_forced_zeros_and_the_known_answers(town01):
    from torchdrivesim_amd import _ops, lanelet2 as L
    from torchdrivesim_amd.infractions import lane_table_set
    state = _agents(town01, 2, 48, 3)
    # absent agents: the present mask multiplies the loss, and the derivative with it
    present = np.random.default_rng(2).random((2, 48)) < 0.5
    lane_set = lane_table_set([town01, town01], torch.device(DEV), 1.0)
    st = torch.from_numpy(state).to(DEV)
    all_out, all_d = _ops.wrong_way(lane_set, st, None, None, math.pi / 2, 1.0, want_dpsi=True)
    out, d = _ops.wrong_way(lane_set, st, None, torch.from_numpy(present).to(DEV), math.pi / 2, 1.0, want_dpsi=True)
    p = torch.from_numpy(present).to(DEV)
    assert not out[~p].any() and not d[~p].any() and torch.equal(out[p], all_out[p]) and torch.equal(d[p], all_d[p]) and bool((all_d[~p] != 0).any())
    # a NaN psi on a lane: every delta is a NaN, the loss is what tds_wrong_way_f32 writes (its bits), and the derivative is a finite 0
    nan_psi = st.clone()
    on_lane = int(torch.nonzero(all_out[1] > 0)[0])
    nan_psi[1, on_lane, 2] = float('nan')
    plain = _ops.wrong_way(lane_set, nan_psi, None, None, math.pi / 2, 1.0)
    out_nan, d_nan = _ops.wrong_way(lane_set, nan_psi, None, None, math.pi / 2, 1.0, want_dpsi=True)
    assert torch.equal(out_nan.view(torch.int32), plain.view(torch.int32)) and d_nan[1, on_lane] == 0 and bool(torch.isfinite(d_nan).all())
    leaf = st.clone().requires_grad_(True)
    _ops.wrong_way_grad(lane_set, leaf, None, p, math.pi / 2, 1.0).sum().backward()
    assert torch.equal(leaf.grad[..., 2], d) and not leaf.grad[..., [0, 1, 3]].any()
    # scenes without a map; no map at all; the one-lanelet map of the reference's known answers, plain and tagged 'parking'
    kat = L.LaneletMap([], np.zeros((0, 3)), [L.make_lanelet(7, KAT_LEFT, KAT_RIGHT)])
    parking = L.LaneletMap([], np.zeros((0, 3)), [L.make_lanelet(7, KAT_LEFT, KAT_RIGHT, {'parking': ''})])
    three = np.concatenate([state, state[:1]], 0)
    three[2, :3] = [[0.5, 0.5, math.pi / 4, 1], [0.5, 0.5, 5 * math.pi / 4, 1], [0.5, 0.5, math.pi / 4 + 2.5, 1]]
    three[2, 3:, :2] = 50.0
    plain, out, dpsi, grad, g = run([None, town01, kat], three, None, math.pi / 2, 1.0)
    assert np.array_equal(out.view(np.int32), plain.view(np.int32)) and not out[0].any() and not dpsi[0].any() and not grad[0].any() and dpsi[1].any()
    assert out[2, 0] == 0 and dpsi[2, 0] == 0
    assert abs(out[2, 1] - 1) <= 1e-6 and abs(dpsi[2, 1] - -math.sin(math.pi)) <= 1e-6, 'against the lane: loss 1, derivative -sin(pi) ~ 0'
    assert abs(out[2, 2] - -math.cos(2.5)) <= 1e-6 and abs(dpsi[2, 2] - -math.sin(-2.5)) <= 1e-6 and dpsi[2, 2] > 0.5
    assert not out[2, 3:].any() and not dpsi[2, 3:].any() and np.array_equal(grad[..., 2], g * dpsi) and not grad[..., [0, 1, 3]].any()
    plain, out, dpsi, grad, g = run([parking, parking, parking], three, None, math.pi / 2, 1.0)
    assert not out.any() and not dpsi.any() and not grad.any(), 'an excluded tag: no directions at all'
    plain, out, dpsi, grad, g = run([None, None, None], three, None, math.pi / 2, 1.0)
    assert not out.any() and not grad.any()
