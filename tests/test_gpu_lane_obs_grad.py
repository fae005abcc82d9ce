"""Differentiable lane observations on the device (csrc/lane_obs_bwd.hip `tds_lane_observations_bwd_multi`; _ops.lane_observations_grad;
Simulator.compute_lanes(differentiable=True)) against the float64 torch-autograd model of their definition (tests/lane_obs_grad_model.py;
include/tdship.h "K8b"), which is fed the very poses and [sin, cos] the kernels read, the index the forward wrote and the incoming
gradients.

The bar is the project's own (tests/test_gpu_backward_float64.py):
    |kernel - float64 model| <= 4 x the largest |float32 model - float64 model| on the same inputs and tensor
-- the yardstick is computed here, from the model alone, and printed beside the kernel's figure (run with -s) before anything is asserted.  It holds
on ALL rows, with no exclusions: the model is fed the forward's own index.  Rows that must be zero are exactly zero.
Set TDS_LANE_OBS_GRAD_OUT=<file> to have the figures written as JSON (that is how profiles/lane_obs_grad_float64.json was made)."""
import json
import os

import numpy as np
import pytest
import torch

import lane_obs_cases as cases
import lane_obs_grad_model as gm
import lane_obs_model as lom
from conftest import GOLDEN
from test_gpu_lane_obs import make_sim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
F32 = np.float32
TENSORS = ('g_xy', 'g_sc')
SPACING, REACH = 4.0, 100.0          # metres: the ring of 70 lanelets is 80 m across, so with K = 32 its rows are full
#: (K, P): one pair; fewer than 64 pairs; pairs that straddle a 64-lane round; 16 full rounds
SHAPES = [(1, 1), (5, 6), (6, 13), (32, 32)]
#: name -> (the maps of the scenes, None for a scene without one; exposed agents; absent agents)
SCENES = {'B4': (('edge', 'chain', 'fork', None), 5, ((0, 4), (2, 1))),
          'B7': (('dead_end', 'loop', 'tagged', 'chain', None, 'fork', 'ring'), 3, ((3, 2), (5, 2)))}
_lanes = {}


def record(label, figures):
    path = os.environ.get('TDS_LANE_OBS_GRAD_OUT')
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[label] = figures
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


def incoming(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def tables_of(maps):
    """the model's table of every scene, made once per map"""
    for m in maps:
        if m is not None and id(m) not in _lanes:
            _lanes[id(m)] = (m, lom.Lanes(m))
    return [None if m is None else _lanes[id(m)][1] for m in maps]


@pytest.fixture(scope='module')
def synthetic():
    return dict({name: make() for name, make in cases.STRUCTURES.items()}, ring=cases.ring())


@pytest.fixture(scope='module')
def scenes(synthetic):
    """name -> (sim, the model's tables, present): per scene the hand poses of the definition's cases in turn (NaN poses among them) and two
    random poses around its map; some agents absent"""
    out = {}
    for name, (maps, A, absent) in SCENES.items():
        rng = np.random.default_rng(len(maps))
        maps = [None if m is None else synthetic[m] for m in maps]
        states = np.zeros((len(maps), A, 4), F32)
        for b, m in enumerate(maps):
            states[b, :, :3] = cases.poses(rng, m if m is not None else synthetic['chain'], A + 2)[2:]        # (not the two ON centre-line points)
            for a in range(A - 2):
                states[b, a, :3] = cases.HAND_POSES[(b * (A - 2) + a) % len(cases.HAND_POSES)]
        present = np.ones(states.shape[:2], bool)
        for b, a in absent:
            present[b, a] = False
        out[name] = (make_sim(maps, states, present), tables_of(maps), present)
    return out


def run(sim, k, p, g_features='random', g_points='random', seed=0, need=('xy', 'sc'), reach=REACH):
    """forward and backward through _ops.lane_observations_grad from leaves of its own -> dict of numpy arrays: the four outputs, the two incoming
    gradients (None for one that was not given), xy, sc, g_xy, g_sc (None for a leaf that did not require grad)"""
    from torchdrivesim_amd import _ops
    A = sim.agent_count
    xy = sim.get_state()[..., :2].detach().clone().requires_grad_('xy' in need)
    sc = sim._heading_sc().detach()[:, :A].clone().requires_grad_('sc' in need)
    features, points, n_valid, index = _ops.lane_observations_grad(sim._lane_tables(torch.device(DEV)), xy, sc, sim.get_present_mask(), k, p, SPACING, reach)
    assert features.requires_grad and points.requires_grad
    for t in (n_valid, index):
        assert not t.requires_grad and t.grad_fn is None and t.dtype == torch.int32
    gf = incoming(features.shape, seed) if isinstance(g_features, str) else g_features
    gp = incoming(points.shape, seed + 1) if isinstance(g_points, str) else g_points
    outs, grads = [o for o, g in ((features, gf), (points, gp)) if g is not None], [g for g in (gf, gp) if g is not None]
    torch.autograd.backward(outs, grads)
    out = dict(features=features.detach().cpu().numpy(), points=points.detach().cpu().numpy(), n_valid=n_valid.cpu().numpy(), index=index.cpu().numpy(),
               gf=None if gf is None else gf.cpu().numpy(), gp=None if gp is None else gp.cpu().numpy(), xy=xy.detach().cpu().numpy(),
               sc=sc.detach().cpu().numpy())
    for key, leaf in (('xy', xy), ('sc', sc)):
        assert (leaf.grad is not None) == (key in need), key
        out['g_' + key] = None if leaf.grad is None else leaf.grad.cpu().numpy()
    return out


def hold(label, lanes, out, p, least=1):
    """every row of both gradient tensors against the model; each tensor's figure is printed before anything is asserted -> filled (B,A,K), valid"""
    m64 = gm.gradients(lanes, out['xy'], out['sc'], out['index'], out['gf'], out['gp'], p, SPACING)
    m32 = gm.gradients(lanes, out['xy'], out['sc'], out['index'], out['gf'], out['gp'], p, SPACING, torch.float32)
    filled, valid = m64[2], m64[3]
    touched = filled.any(-1)
    failures, figures = [], {}
    for i, name in enumerate(TENSORS):
        got, w64, w32 = out[name].astype(np.float64), m64[i], m32[i]
        diff, yard, scale = float(np.abs(got - w64).max()), float(np.abs(w32 - w64).max()), float(np.abs(w64).max())
        print(f'{label} {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}, filled slots {int(filled.sum())} of {filled.size}, valid points {int(valid.sum())} of {valid.size}')
        figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard, largest=scale)
        if not diff <= FACTOR * yard:
            failures.append(f'{label} {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not np.isfinite(got).all():
            failures.append(f'{label} {name}: not finite')
        if (got[~touched] != 0).any() or (w64[~touched] != 0).any():
            failures.append(f'{label} {name}: the row of an observer without a filled slot is not exactly zero')
    figures['filled_slots'], figures['empty_slots'], figures['valid_points'] = int(filled.sum()), int((~filled).sum()), int(valid.sum())
    figures['invalid_points_of_filled_slots'] = int((~valid[filled]).sum())
    record(label, figures)
    assert not failures, '\n'.join(failures)
    assert np.array_equal(filled, out['index'] >= 0) and np.array_equal(valid.sum(-1), out['n_valid']) and filled.sum() >= least, (label, int(filled.sum()))
    return filled, valid


def forward_bits_are_todays(sim, k, p, out, reach=REACH):
    plain = sim.compute_lanes(k=k, n_points=p, spacing=SPACING, max_distance=reach)
    assert plain.features.grad_fn is None and not plain.features.requires_grad and not plain.points.requires_grad
    for name in ('features', 'points', 'n_valid', 'index'):
        assert np.array_equal(out[name].view(np.int32), getattr(plain, name).cpu().numpy().view(np.int32)), name


# ------------------------------------------------------------------------------------------------------------------------ the bar
@pytest.mark.parametrize('k, p', SHAPES)
@pytest.mark.parametrize('name', list(SCENES))
def test_the_synthetic_maps(scenes, name, k, p):
    """one LaneTableSet of several tables with a scene without a map among them (the scene-map path); the hand poses, NaN poses and absent agents;
    the ring's table has more than 64 lanelets, and with K = 32 its rows are full"""
    sim, lanes, present = scenes[name]
    out = run(sim, k, p, seed=k + p)
    forward_bits_are_todays(sim, k, p, out)
    filled, valid = hold(f'{name} K={k} P={p}', lanes, out, p, least=len(lanes))
    nan_pose = np.isnan(out['xy']).any(-1) | np.isnan(out['sc']).any(-1)
    no_map = np.array([l is None for l in lanes])[:, None] | np.zeros_like(present)
    assert nan_pose.sum() >= 2 and (~present).sum() == 2 and no_map.sum() == present.shape[1]
    for rows in (nan_pose, ~present, no_map):
        assert not filled[rows].any() and not out['g_xy'][rows].any() and not out['g_sc'][rows].any()
    assert (~filled).any() and (p == 1 or (~valid[filled]).any()), 'empty slots and invalid points are met'
    if name == 'B7' and k == 32:
        assert filled[6].all(-1).any() and (out['index'][6] >= 64).any(), 'full rows on the ring, lanelets beyond the first 64'


def test_town01():
    """one scene of 8 agents on the golden Town01 map, the defaults"""
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    m = lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    _, states, placed = heuristic_initialize_batch([m], 1, 8, seed=11, device=DEV)
    assert bool(placed.all())
    sim = make_sim([m], states.clone())
    out = run(sim, 6, 8, seed=101, reach=30.0)
    forward_bits_are_todays(sim, 6, 8, out, reach=30.0)
    filled, valid = hold('Town01 K=6 P=8', tables_of([m]), out, 8, least=24)
    assert valid.sum() >= 4 * filled.sum() and np.abs(out['g_xy']).min() > 0


# ------------------------------------------------------------------------------------------------------------------------ exact properties
def test_two_backward_runs_are_equal_and_one_incoming_gradient_alone(scenes):
    sim, lanes, _ = scenes['B7']
    first, again = run(sim, 6, 13, seed=9), run(sim, 6, 13, seed=9)
    for key in TENSORS:
        assert np.array_equal(first[key].view(np.int32), again[key].view(np.int32)) and np.abs(first[key]).max() > 0, key
    gf, gp = torch.from_numpy(first['gf']).to(DEV), torch.from_numpy(first['gp']).to(DEV)
    features_only, points_only = run(sim, 6, 13, g_features=gf, g_points=None), run(sim, 6, 13, g_features=None, g_points=gp)
    assert features_only['gp'] is None and points_only['gf'] is None
    hold('B7 K=6 P=13 g_features alone', lanes, features_only, 13)
    hold('B7 K=6 P=13 g_points alone', lanes, points_only, 13)
    zeros = run(sim, 6, 13, g_features=gf, g_points=torch.zeros_like(gp))
    for key in TENSORS:
        assert np.array_equal(features_only[key], zeros[key]) and not np.array_equal(features_only[key], first[key]), key
    # incoming gradients that are contiguous views at an odd storage offset: the wrapper hands the kernel aligned copies
    odd = lambda g: torch.cat([g.new_zeros(1), g.flatten()])[1:].view(g.shape)
    assert odd(gf).data_ptr() % 16 != 0 and odd(gf).is_contiguous()
    shifted = run(sim, 6, 13, g_features=odd(gf), g_points=odd(gp))
    for key in TENSORS:
        assert np.array_equal(shifted[key].view(np.int32), first[key].view(np.int32)), key
    xy_only = run(sim, 6, 13, seed=9, need=('xy',))
    assert xy_only['g_sc'] is None and np.array_equal(xy_only['g_xy'], first['g_xy'])


def test_a_nan_at_an_empty_slot_or_an_invalid_point_changes_nothing(scenes):
    sim, lanes, _ = scenes['B4']
    first = run(sim, 5, 6, seed=5)
    filled, valid = hold('B4 K=5 P=6 again', lanes, first, 6)
    assert (~filled).sum() >= 20 and (~valid[filled]).sum() >= 5
    gf, gp = first['gf'].copy(), first['gp'].copy()
    gf[~filled] = np.nan
    gf[~filled, 3], gf[~filled, 4] = np.inf, -np.inf
    gp[~valid] = np.nan
    gp[~valid, 1] = np.inf
    again = run(sim, 5, 6, g_features=torch.from_numpy(gf).to(DEV), g_points=torch.from_numpy(gp).to(DEV))
    for key in TENSORS:
        assert np.array_equal(first[key].view(np.int32), again[key].view(np.int32)) and np.isfinite(again[key]).all(), key


def test_garbage_in_the_index_is_never_dereferenced_and_outputs_are_written_in_full(scenes):
    """the entry point itself, with indices out of range and negative (the kernel tests 0 <= l < n of the scene's table before it reads a record,
    and every successor before it follows it) and NaN incoming gradients there, into tensors that held NaN: equal to the model, which treats
    those slots as empty"""
    from torchdrivesim_amd import _native as nat
    sim, lanes, _ = scenes['B4']
    A, K, P = sim.agent_count, 5, 6
    first = run(sim, K, P, seed=6)
    index = torch.from_numpy(first['index']).to(DEV).clone()
    index[1, 0] = torch.tensor([3, -7, 1, 2 ** 31 - 1, 0], dtype=torch.int32)          # chain has lanelets 0 .. 2: 3 is one past the end
    index[2, 3] = torch.tensor([-2 ** 31, 1000000, 2, 70, -1], dtype=torch.int32)
    index[3, 1] = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32)                    # the scene without a map
    gf, gp = incoming((4, A, K, 8), 8), incoming((4, A, K, P, 2), 9)
    bad = (index < 0) | (index > 2)
    gf[bad], gp[bad] = float('nan'), float('nan')
    gf[3], gp[3] = float('inf'), float('nan')
    sc_nan = torch.from_numpy(first['sc']).to(DEV).clone()
    sc_nan[0, 3, 1] = float('nan')                                                     # finite x and y, a NaN cos and a valid index: an empty row all the same
    lane_set = sim._lane_tables(torch.device(DEV))
    assert first['index'][0, 3, 0] == 0
    xy, sc = torch.from_numpy(first['xy']).to(DEV), sc_nan
    outs = [torch.full((4, A, 2), float('nan'), device=DEV) for _ in range(2)]
    nat.call('tds_lane_observations_bwd_multi', torch.device(DEV), lane_set.handle, lane_set.scene_map, xy, sc, index, gf, gp, *outs, 4, A, K, P, SPACING)
    got = dict(first, sc=sc.cpu().numpy(), index=index.cpu().numpy(), gf=gf.cpu().numpy(), gp=gp.cpu().numpy(), g_xy=outs[0].cpu().numpy(), g_sc=outs[1].cpu().numpy())
    m64 = gm.gradients(lanes, got['xy'], got['sc'], got['index'], got['gf'], got['gp'], P, SPACING)
    m32 = gm.gradients(lanes, got['xy'], got['sc'], got['index'], got['gf'], got['gp'], P, SPACING, torch.float32)
    assert m64[2][1, 0].tolist() == [False, False, True, False, True] and m64[2][2, 3].tolist() == [False, False, True, False, False] and not m64[2][3].any()
    for i, key in enumerate(TENSORS):
        assert np.isfinite(got[key]).all(), key
        diff, yard = float(np.abs(got[key] - m64[i]).max()), float(np.abs(m32[i] - m64[i]).max())
        print(f'garbage {key}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g}')
        assert diff <= FACTOR * yard, key
        assert not got[key][3].any() and not got[key][0, 3].any() and np.abs(got[key][1, 0]).max() > 0, key
    # nothing to do: B * A == 0; one incoming gradient NULL through the entry point itself
    nat.call('tds_lane_observations_bwd_multi', torch.device(DEV), lane_set.handle, lane_set.scene_map, None, None, None, None, None, None, None, 4, 0, K, P, SPACING)
    nat.call('tds_lane_observations_bwd_multi', torch.device(DEV), lane_set.handle, lane_set.scene_map, xy, sc, index, None, None, *outs, 4, A, K, P, SPACING)
    assert all(not o.any() for o in outs), 'both gradients NULL: every row is written, as zeros'


# ------------------------------------------------------------------------------------------------------------------------ through the Simulator
def test_through_the_simulator(scenes):
    """a state leaf that requires grad: x, y, psi of the agents' gradient against the model chained with the device's own [sin, cos]; the speed
    column gets exactly 0"""
    sim, lanes, _ = scenes['B7']
    A, k, p = sim.agent_count, 5, 6
    kw = dict(k=k, n_points=p, spacing=SPACING, max_distance=REACH)
    plain = sim.compute_lanes(**kw)
    saved = sim.get_state()
    leaf = saved.detach().clone().requires_grad_(True)
    sim.kinematic_model.set_state(leaf)
    try:
        t = sim.compute_lanes(differentiable=True, **kw)
        assert t.features.requires_grad and t.points.requires_grad and not t.index.requires_grad and not t.n_valid.requires_grad
        assert t.index.grad_fn is None and t.n_valid.grad_fn is None
        for name in ('features', 'points', 'n_valid', 'index'):
            assert torch.equal(getattr(t, name).detach().view(torch.int32), getattr(plain, name).view(torch.int32)), f'{name}: the forward bits are today\'s'
        gf, gp = incoming(t.features.shape, 77), incoming(t.points.shape, 78)
        torch.autograd.backward([t.features, t.points], [gf, gp])
        xy, sc = leaf.detach()[..., :2].cpu().numpy(), sim._heading_sc().detach()[:, :A].cpu().numpy()
        index = t.index.cpu().numpy()
        ref = {}
        for dtype, np_dtype in ((torch.float64, np.float64), (torch.float32, np.float32)):
            g_xy, g_sc, filled, _ = gm.gradients(lanes, xy, sc, index, gf.cpu().numpy(), gp.cpu().numpy(), p, SPACING, dtype)
            ref[dtype] = gm.chain_state(g_xy, g_sc, sc, np_dtype)
        got = leaf.grad.double().cpu().numpy()
        assert got.shape == (7, A, 4) and filled.sum() >= 20 and not got[..., 3].any(), 'the speed is not read'
        failures, figures = [], {}
        for col, name in enumerate(('x', 'y', 'psi')):
            diff = float(np.abs(got[..., col] - ref[torch.float64][..., col]).max())
            yard = float(np.abs(ref[torch.float32][..., col] - ref[torch.float64][..., col]).max())
            print(f'Simulator g_state {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), '
                  f'largest entry {float(np.abs(ref[torch.float64][..., col]).max()):.3g}, filled slots {int(filled.sum())}')
            figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard)
            if not diff <= FACTOR * yard:
                failures.append(f'g_state {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        record('Simulator', figures)
        assert not failures, '\n'.join(failures)
        assert all(np.abs(got[..., col]).max() > 0 for col in range(3)) and not got[~filled.any(-1)].any()
        # the flag off, grad mode off: today's path and today's bits
        for quiet in (sim.compute_lanes(**kw), sim.compute_lanes(differentiable=False, **kw)):
            assert not quiet.features.requires_grad and quiet.features.grad_fn is None and not quiet.points.requires_grad
            assert torch.equal(quiet.features.view(torch.int32), plain.features.view(torch.int32))
        with torch.no_grad():
            quiet = sim.compute_lanes(differentiable=True, **kw)
        assert not quiet.features.requires_grad and quiet.features.grad_fn is None and not quiet.points.requires_grad and quiet.points.grad_fn is None
        assert torch.equal(quiet.points.view(torch.int32), plain.points.view(torch.int32)) and torch.equal(quiet.index, plain.index)
    finally:
        sim.kinematic_model.set_state(saved)
    quiet = sim.compute_lanes(differentiable=True, **kw)                                  # nothing requires grad
    assert not quiet.features.requires_grad and quiet.features.grad_fn is None and not quiet.points.requires_grad and not quiet.index.requires_grad
    assert torch.equal(quiet.features.view(torch.int32), plain.features.view(torch.int32)) and torch.equal(quiet.index, plain.index)


def test_without_a_lanelet_map_nothing_is_recorded():
    states = torch.zeros((2, 3, 4), device=DEV, requires_grad=True)
    for maps in (None, [None, None]):
        sim = make_sim(maps, np.zeros((2, 3, 4), F32))
        sim.kinematic_model.set_state(states)
        obs = sim.compute_lanes(k=3, n_points=5, differentiable=True)
        assert not obs.features.requires_grad and not obs.points.requires_grad and not bool(obs.features.any()) and bool((obs.index == -1).all())
