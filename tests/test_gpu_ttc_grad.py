"""Differentiable time to collision on the device (csrc/ttc_bwd.hip `tds_time_to_collision_bwd_f32`; _ops.time_to_collision_grad;
Simulator.compute_time_to_collision(differentiable=True)) against the float64 torch-autograd model of its definition (tests/ttc_grad_model.py;
include/tdship.h "K9b"), which is fed the very boxes, [sin, cos] and speeds the kernels read, the index the forward wrote and the
incoming gradient.

The bar is the project's own (tests/test_gpu_backward_float64.py):
    |kernel - float64 model| <= 4 x the largest |float32 model - float64 model| on the same inputs and tensor
-- the yardstick is computed here, from the model alone, and printed beside the kernel's figure (run with -s) before anything is asserted.  It holds
on ALL rows: the discrete choices are recomputed from the forward's own binary64 arithmetic, which equals the model's bit for bit
(tests/test_gpu_ttc.py), so no row is borderline.  Rows that must be zero are exactly zero, and so is the psi column.
Set TDS_TTC_GRAD_OUT=<file> to have the figures written as JSON (that is how profiles/ttc_grad_float64.json was made)."""
import json
import os

import numpy as np
import pytest
import torch

import ttc_grad_model as gm
import ttc_model as tm
from conftest import GOLDEN
from test_gpu_range_scan import make_sim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
INF = float('inf')
F32 = np.float32
K, HORIZON, MARGIN = 4, 3.0, 0.25


def record(label, figures):
    path = os.environ.get('TDS_TTC_GRAD_OUT')
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[label] = figures
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


def incoming(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def run(s, A, k, horizon, margin=0.0, visible=None, g=None, seed=0, need=('boxes', 'sc', 'speed')):
    """forward and backward through _ops.time_to_collision_grad from leaves of its own -> dict of numpy arrays: ttc, index, g, g_boxes, g_sc, g_speed
    (None for a leaf that did not require grad)"""
    from torchdrivesim_amd import _ops
    t = {key: torch.from_numpy(v).to(DEV) for key, v in s.items()}
    leaves = {key: t[key].clone().requires_grad_(key in need) for key in ('boxes', 'sc', 'speed')}
    vis = None if visible is None else torch.from_numpy(visible).to(DEV)
    ttc, index = _ops.time_to_collision_grad(leaves['boxes'], leaves['sc'], leaves['speed'], t['present'], A, k, horizon, margin, vis)
    assert ttc.requires_grad and not index.requires_grad and index.grad_fn is None and index.dtype == torch.int32
    g = incoming(ttc.shape, seed) if g is None else g
    torch.autograd.backward([ttc], [g])
    out = dict(ttc=ttc.detach().cpu().numpy(), index=index.cpu().numpy(), g=g.cpu().numpy())
    for key, leaf in leaves.items():
        assert (leaf.grad is not None) == (key in need), key
        out['g_' + key] = None if leaf.grad is None else leaf.grad.cpu().numpy()
    return out


def hold(label, s, out, margin, tensors=('g_boxes', 'g_sc', 'g_speed'), least=1):
    """every row of every gradient tensor against the model; each tensor's figure is printed before anything is asserted -> contributes (B,A,K)"""
    g = np.where(np.isfinite(out['g']), out['g'], 0.0).astype(F32)          # a NaN comes in only where nothing contributes (asserted below)
    m64 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], out['index'], g, margin)
    m32 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], out['index'], g, margin, torch.float32)
    contributes = m64[3]
    assert np.isfinite(out['g'][contributes]).all()
    assert np.array_equal(contributes, (out['index'] >= 0) & (out['ttc'] > 0)), 'a slot contributes exactly where the forward\'s time is above 0'
    touched = np.zeros(s['boxes'].shape[:2], bool)
    b, a, k = np.nonzero(contributes)
    touched[b, a] = True
    touched[b, out['index'][b, a, k]] = True
    failures, figures = [], {}
    for i, name in enumerate(('g_boxes', 'g_sc', 'g_speed')):
        if name not in tensors:
            continue
        got, w64, w32 = out[name].astype(np.float64), m64[i], m32[i]
        diff, yard, scale = float(np.abs(got - w64).max()), float(np.abs(w32 - w64).max()), float(np.abs(w64).max())
        print(f'{label} {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}, contributing slots {int(contributes.sum())} of {contributes.size}, entities touched {int(touched.sum())} of {touched.size}')
        figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard, largest=scale)
        if not diff <= FACTOR * yard:
            failures.append(f'{label} {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not np.isfinite(got).all():
            failures.append(f'{label} {name}: not finite')
        if (got[~touched] != 0).any() or (w64[~touched] != 0).any():
            failures.append(f'{label} {name}: the row of an entity no slot touches is not exactly zero')
    if 'g_boxes' in tensors and (out['g_boxes'][..., 4] != 0).any():
        failures.append(f'{label}: the psi column is not zero')
    figures['contributing_slots'], figures['entities_touched'] = int(contributes.sum()), int(touched.sum())
    record(label, figures)
    assert not failures, '\n'.join(failures)
    assert contributes.sum() >= least, (label, int(contributes.sum()))
    return contributes


def forward_bits_are_todays(s, A, k, horizon, margin, out, visible=None):
    want = tm.time_to_collision(s['boxes'], s['sc'], s['speed'], s['present'], A, k, horizon, margin, visible=visible)
    assert np.array_equal(out['ttc'].view(np.int32), want[0].view(np.int32)) and np.array_equal(out['index'], want[1])


# ------------------------------------------------------------------------------------------------------------------------ the bar
@pytest.mark.parametrize('name, least', [('E6', 7), ('E64', 15), ('E65', 13), ('E130', 17), ('mask100', 1)])
def test_random_scenes(name, least):
    """K = 4, horizon 3 s, margin 0.25 m, a random incoming gradient: one lane per entity and the strided rounds in the forward, one and several
    turns of the lanes over the slots in the backward, absent and NaN entities, duplicated positions (t = 0)"""
    s, A = tm.scenes(name)
    out = run(s, A, K, HORIZON, MARGIN, seed=len(name))
    forward_bits_are_todays(s, A, K, HORIZON, MARGIN, out)
    hold(name, s, out, MARGIN, least=least)
    absent = ~s['present'] | ~np.isfinite(s['speed'])
    assert absent.any() and not out['g_boxes'][absent].any() and not out['g_sc'][absent].any() and not out['g_speed'][absent].any()


def test_three_slices_of_receiving_entities():
    """E = 33: a workgroup takes 16 receiving entities, four per wave, so two full slices and a third with entity 32 alone, which in scene 0 has a
    speed again and is met; A = 17 observers, the forward's second slice with one"""
    s = tm.random_scenes(3318, 2, 17, 33)
    s['speed'][0, 32] = F32(7.5)
    out = run(s, 17, K, HORIZON, MARGIN, seed=33)
    forward_bits_are_todays(s, 17, K, HORIZON, MARGIN, out)
    contributes = hold('E33', s, out, MARGIN, least=47)
    assert (out['index'][0][contributes[0]] == 32).any() and contributes[:, 16].any()


def test_the_visible_mask():
    s, A = tm.scenes('mask40')
    visible = np.random.default_rng(22).random((3, A, 40)) < 0.6
    out = run(s, A, K, HORIZON, MARGIN, visible=visible, seed=40)
    forward_bits_are_todays(s, A, K, HORIZON, MARGIN, out, visible=visible)
    seen = hold('mask40', s, out, MARGIN, least=8)
    plain = run(s, A, K, HORIZON, MARGIN, seed=40)
    assert hold('mask40 unmasked', s, plain, MARGIN, least=32).sum() > seen.sum()


def test_the_entity_limit_with_full_rows():
    """E = 1024, K = 32, no horizon: the forward's rounds, both rows full, 32 KiB of LDS, sixteen turns of the lanes over the 64 x 16 receiving entities"""
    s, A = tm.scenes('E1024')
    out = run(s, A, 32, INF, seed=1024)
    forward_bits_are_todays(s, A, 32, INF, 0.0, out)
    contributes = hold('E1024', s, out, 0.0, least=32)
    assert contributes[0, 0].any() and contributes[0, 1].any()


# ------------------------------------------------------------------------------------------------------------------------ exact properties
def test_a_nan_at_a_slot_that_contributes_nothing_changes_nothing():
    s, A = tm.scenes('E64')
    first = run(s, A, K, HORIZON, MARGIN, seed=5)
    quiet = ~((first['index'] >= 0) & (first['ttc'] > 0))
    assert (first['index'] < 0).any() and ((first['index'] >= 0) & (first['ttc'] == 0)).any(), 'an empty slot and a t = 0 slot'
    g = torch.from_numpy(np.where(quiet, F32(np.nan), first['g'])).to(DEV)
    g[torch.from_numpy(quiet & (first['ttc'] == 0)).to(DEV)] = INF
    again = run(s, A, K, HORIZON, MARGIN, g=g)
    for key in ('g_boxes', 'g_sc', 'g_speed'):
        assert np.array_equal(first[key], again[key]), key


def test_two_backward_runs_are_equal_and_subsets_of_the_inputs_work():
    s, A = tm.scenes('E130')
    first, again = run(s, A, K, HORIZON, MARGIN, seed=9), run(s, A, K, HORIZON, MARGIN, seed=9)
    for key in ('g_boxes', 'g_sc', 'g_speed'):
        assert np.array_equal(first[key], again[key]) and np.abs(first[key]).max() > 0, key
    speed_only = run(s, A, K, HORIZON, MARGIN, seed=9, need=('speed',))
    assert speed_only['g_boxes'] is None and speed_only['g_sc'] is None and np.array_equal(speed_only['g_speed'], first['g_speed'])
    boxes_only = run(s, A, K, HORIZON, MARGIN, seed=9, need=('boxes',))
    assert boxes_only['g_speed'] is None and boxes_only['g_sc'] is None and np.array_equal(boxes_only['g_boxes'], first['g_boxes'])


def ulp32(v):
    return float(np.spacing(np.abs(F32(v))))


@pytest.mark.parametrize('k, e, observer, other', [
    (0, 1, dict(x=-0.05, length=-0.025, speed=-0.115, cos=-1.25), dict(x=0.05, length=-0.025, speed=-0.115, cos=1.25)),
    (1, 3, dict(x=-0.1, length=-0.05, speed=-0.23), dict(x=0.1, width=-0.05, speed=0.0)),
    (2, 4, dict(x=-0.1, length=-0.05, speed=-0.3), dict(x=0.1, length=-0.05, speed=0.3))])
def test_the_definition_cases_by_hand(k, e, observer, other):
    """scene 0 of ttc_model.definition_cases(), horizon 3, margin 0, a unit gradient on one slot of observer 0: each value within one float32 ulp"""
    c = tm.definition_cases()
    g = torch.zeros((2, 3, 4), device=DEV)
    g[0, 0, k] = 1.0
    out = run(c, 3, 4, tm.DEFINITION_HORIZON, 0.0, g=g)
    assert out['index'].tolist() == tm.DEFINITION_INDEX
    rows = lambda j: dict(x=out['g_boxes'][0, j, 0], y=out['g_boxes'][0, j, 1], length=out['g_boxes'][0, j, 2], width=out['g_boxes'][0, j, 3],
                          sin=out['g_sc'][0, j, 0], cos=out['g_sc'][0, j, 1], speed=out['g_speed'][0, j])
    for j, want in ((0, observer), (e, other)):
        got = rows(j)
        for name, v in want.items():
            assert abs(float(got[name]) - v) <= ulp32(v), (j, name, got[name], v)
        assert got['y'] == 0
    others = [j for j in range(6) if j not in (0, e)]
    assert not out['g_boxes'][0, others].any() and not out['g_sc'][0, others].any() and not out['g_speed'][0, others].any()
    assert not out['g_boxes'][1].any() and not out['g_sc'][1].any() and not out['g_speed'][1].any()
    hold(f'definition slot {k}', c, out, 0.0)


def test_garbage_in_the_index_is_never_dereferenced_and_outputs_are_written_in_full():
    """the entry point itself, with indices out of range, the observer's own and NaN incoming gradients there, into tensors that held NaN"""
    from torchdrivesim_amd import _native as nat
    c = tm.definition_cases()
    t = {key: torch.from_numpy(v).to(DEV) for key, v in c.items()}
    index = torch.tensor(tm.DEFINITION_INDEX, dtype=torch.int32, device=DEV)
    index[0, 2] = torch.tensor([6, -7, 2, 2 ** 31 - 1], dtype=torch.int32)
    index[1, 0] = torch.tensor([-2 ** 31, 1000000, 0, 6], dtype=torch.int32)
    g = torch.ones((2, 3, 4), device=DEV)
    g[0, 2], g[1] = float('nan'), float('nan')
    outs = [torch.full(shape, float('nan'), device=DEV) for shape in ((2, 6, 5), (2, 6, 2), (2, 6))]
    nat.call('tds_time_to_collision_bwd_f32', torch.device(DEV), t['boxes'], t['sc'], t['speed'], index, g, *outs, 2, 3, 6, 4, 0.0)
    got = dict(index=index.cpu().numpy(), g=g.cpu().numpy(), g_boxes=outs[0].cpu().numpy(), g_sc=outs[1].cpu().numpy(), g_speed=outs[2].cpu().numpy())
    m64 = gm.scene_gradients(c['boxes'], c['sc'], c['speed'], got['index'], np.where(np.isfinite(got['g']), got['g'], 0.0), 0.0)
    assert not m64[3][1].any() and not m64[3][0, 2].any() and m64[3][0, 0, :3].all()
    for i, key in enumerate(('g_boxes', 'g_sc', 'g_speed')):
        assert np.isfinite(got[key]).all() and not got[key][1].any(), key
        assert np.abs(got[key] - m64[i]).max() <= 1e-6, key
    # nothing to do and no rows: B * E == 0 and A == 0
    nat.call('tds_time_to_collision_bwd_f32', torch.device(DEV), None, None, None, None, None, None, None, None, 0, 0, 4, 1, 0.0)
    nat.call('tds_time_to_collision_bwd_f32', torch.device(DEV), t['boxes'], t['sc'], t['speed'], None, None, *outs, 2, 0, 6, 4, 0.0)
    assert all(not o.any() for o in outs), 'A == 0: every row is written, as zeros'


# ------------------------------------------------------------------------------------------------------------------------ through the Simulator
@pytest.fixture(scope='module')
def town01():
    """what test_gpu_range_scan.make_sim takes, with Town01 alone"""
    import bench
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.mesh import BirdviewMesh
    lanes = lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    v, f, vc, c = bench.load_town01()
    mesh = BirdviewMesh(verts=torch.from_numpy(v)[None], faces=torch.from_numpy(f.astype(np.int64))[None], categories=c, colors={}, zs={},
                        vert_category=torch.from_numpy(vc.astype(np.int64))[None])
    return [lanes], [mesh], [(v, f.astype(np.int64))]


def moving(states, present):
    """everybody drives at 4 .. 15 m/s; agent 1 of scene 0 stands on agent 0; agent 2 of scene 0 crawls 30 m ahead of agent 3, on its course; agent 5
    of scene 1 comes head-on at agent 4 from 40 m, a little to the side and turned; one NPC is absent"""
    B, E = states.shape[:2]
    states[..., 3] = 4.0 + 11.0 * torch.arange(B * E, device=states.device).reshape(B, E) / (B * E)
    states[0, 1, :2] = states[0, 0, :2]
    psi = states[0, 3, 2]
    states[0, 2, :2] = states[0, 3, :2] + 30.0 * torch.stack([torch.cos(psi), torch.sin(psi)])
    states[0, 2, 2] = psi
    states[0, 2, 3], states[0, 3, 3] = 2.0, 12.0
    psi = states[1, 4, 2]
    states[1, 5, :2] = states[1, 4, :2] + 40.0 * torch.stack([torch.cos(psi), torch.sin(psi)]) - 0.4 * torch.stack([-torch.sin(psi), torch.cos(psi)])
    states[1, 5, 2] = psi + 3.1                      # 0.04 rad off head-on: it drifts some 0.8 m to the left on its 20 m, from 0.4 m to the right
    present[1, 9] = False


@pytest.fixture(scope='module')
def sim(town01):
    """Town01, 3 scenes x (8 agents + 4 NPCs) placed by heuristic_initialize_batch"""
    return make_sim(town01, [0, 0, 0], 8, seed=17, npc=4, edit=moving)


def model_inputs(sim):
    """exactly what compute_time_to_collision hands to the kernels, as numpy arrays"""
    st = sim.get_all_agent_state().detach()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1)
    return dict(boxes=boxes.cpu().numpy(), sc=sim._heading_sc().detach().cpu().numpy(), speed=st[..., 3].contiguous().cpu().numpy(),
                present=sim.get_all_agent_present_mask().cpu().numpy())


def test_through_the_simulator(sim):
    """a state leaf that requires grad: x, y, psi, v of the agents' gradient against the model chained with the device's own [sin, cos]"""
    A, k, margin = 8, 6, 0.25
    plain = sim.compute_time_to_collision(k=k, horizon=INF, margin=margin)
    saved = sim.get_state()
    leaf = saved.detach().clone().requires_grad_(True)
    sim.kinematic_model.set_state(leaf)
    try:
        t = sim.compute_time_to_collision(k=k, horizon=INF, margin=margin, differentiable=True)
        assert t.ttc.requires_grad and not t.index.requires_grad
        assert torch.equal(t.ttc.detach().view(torch.int32), plain.ttc.view(torch.int32)) and torch.equal(t.index, plain.index), 'the forward bits are today\'s'
        g = incoming(t.ttc.shape, 77)
        torch.autograd.backward([t.ttc], [g])
        s = model_inputs(sim)
        index, gn = t.index.cpu().numpy(), g.cpu().numpy()
        failures = []
        figures = {}
        ref = {}
        for dtype, np_dtype in ((torch.float64, np.float64), (torch.float32, np.float32)):
            gb, gsc, gv, contributes = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], index, gn, margin, dtype)
            ref[dtype] = gm.chain_state(gb, gsc, gv, s['sc'], np_dtype)[:, :A]
        got = leaf.grad.double().cpu().numpy()
        # by construction: the crawler and the car behind it, the head-on pair, each seen from both sides
        assert got.shape == (3, A, 4) and contributes.sum() >= 4
        assert contributes[0, 2].any() and contributes[0, 3].any() and contributes[1, 4].any() and contributes[1, 5].any()
        for col, name in enumerate(('x', 'y', 'psi', 'v')):
            diff = float(np.abs(got[..., col] - ref[torch.float64][..., col]).max())
            yard = float(np.abs(ref[torch.float32][..., col] - ref[torch.float64][..., col]).max())
            print(f'Simulator g_state {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), '
                  f'largest entry {float(np.abs(ref[torch.float64][..., col]).max()):.3g}, contributing slots {int(contributes.sum())}')
            figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard)
            if not diff <= FACTOR * yard:
                failures.append(f'g_state {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        record('Simulator', figures)
        assert not failures, '\n'.join(failures)
        assert np.abs(got[..., 2]).max() > 0 and np.abs(got[..., 3]).max() > 0
        # the flag off, grad mode off, or nothing requiring grad: today's path and today's bits
        for quiet in (sim.compute_time_to_collision(k=k, horizon=INF, margin=margin), sim.compute_time_to_collision(k=k, horizon=INF, margin=margin, differentiable=False)):
            assert not quiet.ttc.requires_grad and quiet.ttc.grad_fn is None and torch.equal(quiet.ttc.view(torch.int32), plain.ttc.view(torch.int32))
        with torch.no_grad():
            quiet = sim.compute_time_to_collision(k=k, horizon=INF, margin=margin, differentiable=True)
        assert not quiet.ttc.requires_grad and torch.equal(quiet.ttc.view(torch.int32), plain.ttc.view(torch.int32)) and torch.equal(quiet.index, plain.index)
    finally:
        sim.kinematic_model.set_state(saved)
    quiet = sim.compute_time_to_collision(k=k, horizon=INF, margin=margin, differentiable=True)           # nothing requires grad
    assert not quiet.ttc.requires_grad and quiet.ttc.grad_fn is None and not quiet.index.requires_grad
    assert torch.equal(quiet.ttc.view(torch.int32), plain.ttc.view(torch.int32)) and torch.equal(quiet.index, plain.index)


def test_a_size_that_requires_grad_gets_its_gradient(sim):
    saved = sim.agent_size
    size = saved.detach().clone().requires_grad_(True)
    sim.agent_size = size
    try:
        t = sim.compute_time_to_collision(k=2, horizon=INF, differentiable=True)
        assert t.ttc.requires_grad
        finite = torch.isfinite(t.ttc)
        torch.where(finite, t.ttc, torch.zeros_like(t.ttc)).sum().backward()
        assert size.grad.shape == saved.shape and bool(torch.isfinite(size.grad).all()) and float(size.grad.min()) < 0 and float(size.grad.max()) <= 0, \
            'a larger box touches sooner'
    finally:
        sim.agent_size = saved
