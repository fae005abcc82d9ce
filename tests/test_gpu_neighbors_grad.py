"""Differentiable neighbour observations on the device (csrc/neighbors_bwd.hip `tds_neighbors_bwd_f32`; _ops.neighbors_grad;
Simulator.compute_neighbors(differentiable=True)) against the float64 torch-autograd model of their definition (tests/neighbors_grad_model.py;
include/tdship.h "K6b"), which is fed the very boxes, [sin, cos] and speeds the kernels read, the index the forward wrote and the
incoming gradient.

The bar is the project's own (tests/test_gpu_backward_float64.py):
    |kernel - float64 model| <= 4 x the largest |float32 model - float64 model| on the same inputs and tensor
-- the yardstick is computed here, from the model alone, and printed beside the kernel's figure (run with -s) before anything is asserted.  It holds
on ALL rows, with no exclusions: the model is fed the forward's own index.  Rows that must be zero are exactly zero, and so is the psi column.
Set TDS_NEIGHBORS_GRAD_OUT=<file> to have the figures written as JSON (that is how profiles/neighbors_grad_float64.json was made)."""
import json
import os

import numpy as np
import pytest
import torch

import neighbors_grad_model as gm
import neighbors_model as nm
from conftest import GOLDEN
from test_gpu_range_scan import make_sim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
INF = float('inf')
F32 = np.float32
TENSORS = ('g_boxes', 'g_sc', 'g_speed')


def record(label, figures):
    path = os.environ.get('TDS_NEIGHBORS_GRAD_OUT')
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[label] = figures
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


def incoming(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def run(s, A, k, reach, visible=None, g=None, seed=0, need=('boxes', 'sc', 'speed')):
    """forward and backward through _ops.neighbors_grad from leaves of its own -> dict of numpy arrays: features, index, g, g_boxes, g_sc, g_speed
    (None for a leaf that did not require grad)"""
    from torchdrivesim_amd import _ops
    t = {key: torch.from_numpy(v).to(DEV) for key, v in s.items()}
    leaves = {key: t[key].clone().requires_grad_(key in need) for key in ('boxes', 'sc', 'speed')}
    vis = None if visible is None else torch.from_numpy(visible).to(DEV)
    features, index = _ops.neighbors_grad(leaves['boxes'], leaves['sc'], leaves['speed'], t['present'], A, k, reach, vis)
    assert features.requires_grad and not index.requires_grad and index.grad_fn is None and index.dtype == torch.int32
    g = incoming(features.shape, seed) if g is None else g
    torch.autograd.backward([features], [g])
    out = dict(features=features.detach().cpu().numpy(), index=index.cpu().numpy(), g=g.cpu().numpy())
    for key, leaf in leaves.items():
        assert (leaf.grad is not None) == (key in need), key
        out['g_' + key] = None if leaf.grad is None else leaf.grad.cpu().numpy()
    return out


def hold(label, s, out, tensors=TENSORS, least=1):
    """every row of every gradient tensor against the model; each tensor's figure is printed before anything is asserted -> filled (B,A,K)"""
    m64 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], out['index'], out['g'])
    m32 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], out['index'], out['g'], torch.float32)
    filled = m64[3]
    E = s['boxes'].shape[1]
    touched = gm.touched(filled, out['index'], E)
    failures, figures = [], {}
    for i, name in enumerate(TENSORS):
        if name not in tensors:
            continue
        got, w64, w32 = out[name].astype(np.float64), m64[i], m32[i]
        diff, yard, scale = float(np.abs(got - w64).max()), float(np.abs(w32 - w64).max()), float(np.abs(w64).max())
        print(f'{label} {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}, filled slots {int(filled.sum())} of {filled.size}, entities touched {int(touched.sum())} of {touched.size}')
        figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard, largest=scale)
        if not diff <= FACTOR * yard:
            failures.append(f'{label} {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not np.isfinite(got).all():
            failures.append(f'{label} {name}: not finite')
        if (got[~touched] != 0).any() or (w64[~touched] != 0).any():
            failures.append(f'{label} {name}: the row of an entity no slot touches is not exactly zero')
    if 'g_boxes' in tensors and (out['g_boxes'][..., 4] != 0).any():
        failures.append(f'{label}: the psi column is not zero')
    figures['filled_slots'], figures['empty_slots'], figures['entities_untouched'] = int(filled.sum()), int((~filled).sum()), int((~touched).sum())
    record(label, figures)
    assert not failures, '\n'.join(failures)
    assert np.array_equal(filled, out['index'] >= 0) and filled.sum() >= least, (label, int(filled.sum()))
    return filled


def forward_bits_are_todays(s, A, k, reach, out, visible=None):
    want = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], A, k, reach, visible=visible)
    assert np.array_equal(out['features'].view(np.int32), want[0].view(np.int32)) and np.array_equal(out['index'], want[1])


def case(name):
    seed, B, A, E, K, reach = gm.CASES[name]
    return nm.random_scenes(seed, B, A, E), A, K, reach


# ------------------------------------------------------------------------------------------------------------------------ the bar
@pytest.mark.parametrize('name', list(gm.CASES))
def test_random_scenes(name):
    """fewer entities than lanes; one lane per entity; the forward's rounds path; three slices of receiving entities, the third with entity 32
    alone; several turns of the lanes over the slots; the entity limit and the limit of K -- with absent entities and duplicated positions"""
    s, A, K, reach = case(name)
    out = run(s, A, K, reach, seed=len(name))
    forward_bits_are_todays(s, A, K, reach, out)
    filled = hold(name, s, out, least=gm.FILLED[name])
    absent = ~s['present']
    if name != 'E1024':
        assert absent.any() and (~filled).any()
    assert not out['g_boxes'][absent].any() and not out['g_sc'][absent].any() and not out['g_speed'][absent].any()
    if name == 'E33':
        assert (out['index'][filled] == 32).any() and filled[:, 16].any(), 'entity 32 is met, and the forward\'s second slice observes'


def test_an_entity_with_a_nan_pose_gets_zeros():
    s, A, K, reach = case('E64')
    s['boxes'][0, 5, 0] = np.nan
    s['boxes'][1, 7, 1] = np.inf
    out = run(s, A, K, reach, seed=11)
    forward_bits_are_todays(s, A, K, reach, out)
    hold('E64 with a NaN pose', s, out, least=400)
    for b, j in ((0, 5), (1, 7)):
        assert not (out['index'][b] == j).any() and not (out['index'][b, j] >= 0).any()
        assert not out['g_boxes'][b, j].any() and not out['g_sc'][b, j].any() and out['g_speed'][b, j] == 0


def test_the_visible_mask():
    s = nm.random_scenes(40, 3, 10, 40)
    visible = np.random.default_rng(22).random((3, 10, 40)) < 0.6
    out = run(s, 10, 4, 50.0, visible=visible, seed=40)
    forward_bits_are_todays(s, 10, 4, 50.0, out, visible=visible)
    seen = hold('mask40', s, out, least=90)
    plain = run(s, 10, 4, 50.0, seed=40)
    assert hold('mask40 unmasked', s, plain, least=100).sum() > seen.sum()


# ------------------------------------------------------------------------------------------------------------------------ exact properties
def test_a_nan_at_an_empty_slot_changes_nothing():
    s, A, K, reach = case('E64')
    first = run(s, A, K, reach, seed=5)
    empty = first['index'] < 0
    assert empty.sum() >= 56
    g = first['g'].copy()
    g[empty] = np.nan
    g[empty, 3] = np.inf
    g[empty, 4] = -np.inf
    again = run(s, A, K, reach, g=torch.from_numpy(g).to(DEV))
    for key in TENSORS:
        assert np.array_equal(first[key], again[key]) and np.isfinite(again[key]).all(), key
    hold('E64 with NaN at the empty slots', s, again)


def test_two_backward_runs_are_equal_and_subsets_of_the_inputs_work():
    s, A, K, reach = case('E130')
    first, again = run(s, A, K, reach, seed=9), run(s, A, K, reach, seed=9)
    for key in TENSORS:
        assert np.array_equal(first[key], again[key]) and np.abs(first[key]).max() > 0, key
    speed_only = run(s, A, K, reach, seed=9, need=('speed',))
    assert speed_only['g_boxes'] is None and speed_only['g_sc'] is None and np.array_equal(speed_only['g_speed'], first['g_speed'])
    boxes_only = run(s, A, K, reach, seed=9, need=('boxes',))
    assert boxes_only['g_speed'] is None and boxes_only['g_sc'] is None and np.array_equal(boxes_only['g_boxes'], first['g_boxes'])


def test_the_definition_cases():
    """neighbors_model.definition_cases(): the index by hand, every slot with a gradient of its own"""
    c = nm.definition_cases()
    out = run(c, 3, 4, nm.DEFINITION_MAX_DISTANCE, seed=4)
    assert out['index'].tolist() == nm.DEFINITION_INDEX
    forward_bits_are_todays(c, 3, 4, nm.DEFINITION_MAX_DISTANCE, out)
    hold('definition cases', c, out, least=10)
    for key in TENSORS:                                     # scene 1: the absent observer 0, the NaN pose 3 and the absent NPC 4
        assert not out[key][1, [0, 3, 4]].any(), key


def test_garbage_in_the_index_is_never_dereferenced_and_outputs_are_written_in_full():
    """the entry point itself, with indices out of range, the observer's own and NaN incoming gradients there, into tensors that held NaN"""
    from torchdrivesim_amd import _native as nat
    c = nm.definition_cases()
    t = {key: torch.from_numpy(v).to(DEV) for key, v in c.items()}
    index = torch.tensor(nm.DEFINITION_INDEX, dtype=torch.int32, device=DEV)
    index[0, 2] = torch.tensor([5, -7, 2, 2 ** 31 - 1], dtype=torch.int32)
    index[1, 0] = torch.tensor([-2 ** 31, 1000000, 0, 5], dtype=torch.int32)
    g = incoming((2, 3, 4, 8), 8)
    g[0, 2], g[1, 0] = float('nan'), float('nan')
    g[index < 0] = float('nan')
    outs = [torch.full(shape, float('nan'), device=DEV) for shape in ((2, 5, 5), (2, 5, 2), (2, 5))]
    nat.call('tds_neighbors_bwd_f32', torch.device(DEV), t['boxes'], t['sc'], t['speed'], index, g, *outs, 2, 3, 5, 4)
    got = dict(index=index.cpu().numpy(), g=g.cpu().numpy(), g_boxes=outs[0].cpu().numpy(), g_sc=outs[1].cpu().numpy(), g_speed=outs[2].cpu().numpy())
    m64 = gm.scene_gradients(c['boxes'], c['sc'], c['speed'], got['index'], got['g'])
    m32 = gm.scene_gradients(c['boxes'], c['sc'], c['speed'], got['index'], got['g'], torch.float32)
    assert not m64[3][0, 2].any() and not m64[3][1, 0].any() and m64[3][0, 0, :3].all() and m64[3].sum() == 9
    for i, key in enumerate(TENSORS):
        assert np.isfinite(got[key]).all(), key
        diff, yard = float(np.abs(got[key] - m64[i]).max()), float(np.abs(m32[i] - m64[i]).max())
        print(f'garbage {key}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g}')
        assert diff <= FACTOR * yard, key
        assert not got[key][1, [0, 3, 4]].any(), key
    # nothing to do and no rows: B * E == 0 and A == 0
    nat.call('tds_neighbors_bwd_f32', torch.device(DEV), None, None, None, None, None, None, None, None, 0, 0, 4, 1)
    nat.call('tds_neighbors_bwd_f32', torch.device(DEV), t['boxes'], t['sc'], t['speed'], None, None, *outs, 2, 0, 5, 4)
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
    """everybody drives at 4 .. 15 m/s; agent 1 of scene 0 stands on agent 0; one NPC is absent"""
    B, E = states.shape[:2]
    states[..., 3] = 4.0 + 11.0 * torch.arange(B * E, device=states.device).reshape(B, E) / (B * E)
    states[0, 1, :2] = states[0, 0, :2]
    present[1, 9] = False


@pytest.fixture(scope='module')
def sim(town01):
    """Town01, 3 scenes x (8 agents + 4 NPCs) placed by heuristic_initialize_batch"""
    return make_sim(town01, [0, 0, 0], 8, seed=17, npc=4, edit=moving)


def model_inputs(sim):
    """exactly what compute_neighbors hands to the kernels, as numpy arrays"""
    st = sim.get_all_agent_state().detach()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1)
    return dict(boxes=boxes.cpu().numpy(), sc=sim._heading_sc().detach().cpu().numpy(), speed=st[..., 3].contiguous().cpu().numpy(),
                present=sim.get_all_agent_present_mask().cpu().numpy())


REACH = 300.0           # metres: Town01 is some 400 m across, so most rows are full


def test_through_the_simulator(sim):
    """a state leaf that requires grad: x, y, psi, v of the agents' gradient against the model chained with the device's own [sin, cos]"""
    A, k = 8, 6
    plain = sim.compute_neighbors(k=k, max_distance=REACH)
    assert plain.features.grad_fn is None and not plain.features.requires_grad
    saved = sim.get_state()
    leaf = saved.detach().clone().requires_grad_(True)
    sim.kinematic_model.set_state(leaf)
    try:
        t = sim.compute_neighbors(k=k, max_distance=REACH, differentiable=True)
        assert t.features.requires_grad and not t.index.requires_grad
        assert torch.equal(t.features.detach().view(torch.int32), plain.features.view(torch.int32)) and torch.equal(t.index, plain.index), \
            'the forward bits are today\'s'
        g = incoming(t.features.shape, 77)
        torch.autograd.backward([t.features], [g])
        s = model_inputs(sim)
        index, gn = t.index.cpu().numpy(), g.cpu().numpy()
        failures, figures, ref = [], {}, {}
        for dtype, np_dtype in ((torch.float64, np.float64), (torch.float32, np.float32)):
            gb, gsc, gv, filled = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], index, gn, dtype)
            ref[dtype] = gm.chain_state(gb, gsc, gv, s['sc'], np_dtype)[:, :A]
        got = leaf.grad.double().cpu().numpy()
        assert got.shape == (3, A, 4) and filled.sum() >= 3 * A * 3 and (index[filled] >= A).any(), 'NPCs are met too'
        for col, name in enumerate(('x', 'y', 'psi', 'v')):
            diff = float(np.abs(got[..., col] - ref[torch.float64][..., col]).max())
            yard = float(np.abs(ref[torch.float32][..., col] - ref[torch.float64][..., col]).max())
            print(f'Simulator g_state {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), '
                  f'largest entry {float(np.abs(ref[torch.float64][..., col]).max()):.3g}, filled slots {int(filled.sum())}')
            figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard)
            if not diff <= FACTOR * yard:
                failures.append(f'g_state {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        record('Simulator', figures)
        assert not failures, '\n'.join(failures)
        assert all(np.abs(got[..., col]).max() > 0 for col in range(4))
        # the flag off, grad mode off, or nothing requiring grad: today's path and today's bits
        for quiet in (sim.compute_neighbors(k=k, max_distance=REACH), sim.compute_neighbors(k=k, max_distance=REACH, differentiable=False)):
            assert not quiet.features.requires_grad and quiet.features.grad_fn is None
            assert torch.equal(quiet.features.view(torch.int32), plain.features.view(torch.int32))
        with torch.no_grad():
            quiet = sim.compute_neighbors(k=k, max_distance=REACH, differentiable=True)
        assert not quiet.features.requires_grad and quiet.features.grad_fn is None
        assert torch.equal(quiet.features.view(torch.int32), plain.features.view(torch.int32)) and torch.equal(quiet.index, plain.index)
    finally:
        sim.kinematic_model.set_state(saved)
    quiet = sim.compute_neighbors(k=k, max_distance=REACH, differentiable=True)           # nothing requires grad
    assert not quiet.features.requires_grad and quiet.features.grad_fn is None and not quiet.index.requires_grad
    assert torch.equal(quiet.features.view(torch.int32), plain.features.view(torch.int32)) and torch.equal(quiet.index, plain.index)


def test_a_size_that_requires_grad_gets_its_gradient(sim):
    """length and width are copied into the slots an entity fills: its gradient is exactly the sum of what comes in there"""
    saved = sim.agent_size
    size = saved.detach().clone().requires_grad_(True)
    sim.agent_size = size
    try:
        t = sim.compute_neighbors(k=3, max_distance=REACH, differentiable=True)
        assert t.features.requires_grad and t.features.grad_fn is not None
        g = incoming(t.features.shape, 78)
        torch.autograd.backward([t.features], [g])
        index, gn = t.index.cpu().numpy(), g.cpu().numpy().astype(np.float64)
        want = np.zeros(tuple(size.shape))
        b, a, k = np.nonzero(index >= 0)
        exposed = index[b, a, k] < size.shape[1]
        np.add.at(want, (b[exposed], index[b, a, k][exposed]), gn[b, a, k][exposed][:, 6:8])
        assert size.grad.shape == saved.shape and exposed.sum() >= 20 and np.abs(want).max() > 0
        assert np.array_equal(size.grad.cpu().numpy(), want.astype(F32)), 'the float64 sum of a few float32 values is exact, whatever its order'
    finally:
        sim.agent_size = saved
