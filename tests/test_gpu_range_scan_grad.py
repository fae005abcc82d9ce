"""Differentiable range scans on the device (csrc/scan_bwd.hip `tds_range_scan_bwd_f32` / `_multi`; _ops.range_scan_grad, _ops.range_scan_witness)
against the float64 torch-autograd model of their definition (tests/range_scan_grad_model.py; include/tdship.h "K5b"), which is
fed the very boxes, [sin, cos] and rays the kernels read, the kernel's own witness (which rectangle side and which road edge a ray ends on) and
the incoming gradients.

The bar is the project's own (tests/test_gpu_backward_float64.py):
    |kernel - float64 model| <= 4 x the largest |float32 model - float64 model| on the same inputs and tensor
-- the yardstick is computed here, from the model alone, and printed beside the kernel's figure (run with -s) before anything is asserted.  It holds
on ALL rows, with no exclusions.  The witness itself is held to the forward (`hit`) and to the brute-force float64 model of K5
(tests/range_scan_model.py): the reported edge crosses the ray where the model's road stretch ends.
Set TDS_RANGE_SCAN_GRAD_OUT=<file> to have the figures written as JSON (that is how profiles/range_scan_grad_float64.json was made)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import range_scan_grad_model as gm
import range_scan_model as rm
from test_gpu_range_scan import hand_placed, make_sim, model_inputs, towns  # noqa: F401  (towns: the module's fixture)
from test_range_scan_model import GPU_BAR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
EXCEPTION_SHARE = 1e-4
TENSORS = ('g_boxes', 'g_sc', 'g_ray_sc')


def record(label, figures):
    path = os.environ.get('TDS_RANGE_SCAN_GRAD_OUT')
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[label] = figures
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


def incoming(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def run(smap, s, max_range, gap=0.02, want_agents=True, g=None, seed=0, need=('boxes', 'sc', 'ray_sc')):
    """forward and backward through _ops.range_scan_grad from leaves of its own -> dict of numpy arrays: agents, road, hit, choice, road_edge,
    g_agent, g_road, g_boxes, g_sc, g_ray_sc (None for a leaf that did not require grad)"""
    from torchdrivesim_amd import _ops
    t = {key: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for key, v in s.items()}
    A = s['ray_sc'].shape[1]
    leaves = {key: t[key].clone().requires_grad_(key in need) for key in ('boxes', 'sc', 'ray_sc')}
    agents, road, hit = _ops.range_scan_grad(smap, leaves['boxes'], leaves['sc'], t['present'], leaves['ray_sc'], A, max_range, gap, want_agents)
    assert agents.requires_grad and road.requires_grad and not hit.requires_grad and hit.grad_fn is None and hit.dtype == torch.int32
    plain = _ops.range_scan(smap, t['boxes'], t['sc'], t['present'], t['ray_sc'], A, max_range, gap, want_agents=want_agents)
    assert torch.equal(agents.detach().view(torch.int32), plain[0].view(torch.int32)) and torch.equal(road.detach().view(torch.int32), plain[1].view(torch.int32))
    assert torch.equal(hit, plain[2]) and not plain[0].requires_grad and plain[1].grad_fn is None, 'the forward bits are today\'s'
    g = (incoming(agents.shape, seed), incoming(road.shape, seed + 1000)) if g is None else g
    torch.autograd.backward([agents, road], list(g))
    choice, road_edge = _ops.range_scan_witness(smap, t['boxes'], t['sc'], t['present'], t['ray_sc'], A, max_range, gap, want_agents)
    out = dict(agents=agents.detach().cpu().numpy(), road=road.detach().cpu().numpy(), hit=hit.cpu().numpy(), choice=choice.cpu().numpy(),
               road_edge=road_edge.cpu().numpy(), g_agent=g[0].cpu().numpy(), g_road=g[1].cpu().numpy())
    for key, leaf in leaves.items():
        assert (leaf.grad is not None) == (key in need), key
        out['g_' + key] = None if leaf.grad is None else leaf.grad.cpu().numpy()
    return out


def hold(label, s, out, max_range, tensors=TENSORS, least_agent=0, least_road=0, has_road=True, want_agents=True):
    """the witness against the forward, then every row of every gradient tensor against the model; each tensor's figure is printed before
    anything is asserted -> (live_agent, live_road)"""
    choice, edge, hit = out['choice'], out['road_edge'], out['hit']
    assert choice.dtype == np.int32 and edge.dtype == np.float32
    assert np.array_equal(choice[..., 0][hit >= 0], hit[hit >= 0]), 'where hit names an entity, the witness names the same'
    road_live = (out['road'] > 0) & (out['road'] < np.float32(max_range)) if has_road else np.zeros(hit.shape, bool)
    finite = np.isfinite(edge).all(-1)
    assert np.array_equal(finite, road_live), f'{label}: {int((road_live & ~finite).sum())} rays that end on the road have no edge'
    assert np.isnan(edge[~finite]).all()
    agent_live = (out['agents'] > 0) & (out['agents'] < np.float32(max_range)) if want_agents else np.zeros(hit.shape, bool)
    if want_agents:
        assert np.array_equal(choice[..., 0] >= 0, out['agents'] < np.float32(max_range)), 'an entity wherever agents is below max_range'
        assert np.array_equal((choice[..., 0] >= 0) & (choice[..., 1] > 0), agent_live), 'a slab binds wherever 0 < agents < max_range'
    else:
        assert (choice[..., 0] == -1).all() and (choice[..., 1] == 0).all()
    args = (s['boxes'], s['sc'], s['ray_sc'], choice, edge, out['g_agent'] if want_agents else None, out['g_road'] if has_road else None)
    m64, m32 = gm.scene_gradients(*args), gm.scene_gradients(*args, torch.float32)
    assert np.array_equal(m64[3], agent_live) and np.array_equal(m64[4], road_live)
    E = s['boxes'].shape[1]
    touched = gm.touched(choice, agent_live, road_live, E)
    failures, figures = [], {}
    for i, name in enumerate(TENSORS):
        if name not in tensors or out[name] is None:
            continue
        got, w64, w32 = out[name].astype(np.float64), m64[i], m32[i]
        diff, yard, scale = float(np.abs(got - w64).max()), float(np.abs(w32 - w64).max()), float(np.abs(w64).max())
        print(f'{label} {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}, live rays: agents {int(agent_live.sum())}, road {int(road_live.sum())} of {hit.size}, entities touched {int(touched.sum())} of '
              f'{touched.size}')
        figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard, largest=scale)
        if not diff <= FACTOR * yard:
            failures.append(f'{label} {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not np.isfinite(got).all():
            failures.append(f'{label} {name}: not finite')
        if name != 'g_ray_sc' and ((got[~touched] != 0).any() or (w64[~touched] != 0).any()):
            failures.append(f'{label} {name}: the row of an entity no ray touches is not exactly zero')
        if name == 'g_ray_sc' and (got[~(agent_live | road_live)] != 0).any():
            failures.append(f'{label} {name}: a dead ray got a gradient')
        if name != 'g_ray_sc' and (got[~s['present']] != 0).any():
            failures.append(f'{label} {name}: an absent entity got a gradient')
    if 'g_boxes' in tensors and out['g_boxes'] is not None and (out['g_boxes'][..., 4] != 0).any():
        failures.append(f'{label}: the psi column is not zero')
    figures['live_agent_rays'], figures['live_road_rays'], figures['rays'] = int(agent_live.sum()), int(road_live.sum()), int(hit.size)
    record(label, figures)
    assert not failures, '\n'.join(failures)
    assert agent_live.sum() >= least_agent and road_live.sum() >= least_road, (label, int(agent_live.sum()), int(road_live.sum()))
    return agent_live, road_live


def edges_end_the_models_road(label, out, s, raw, which, max_range, gap=0.02):
    """every reported edge: its float64 crossing with the ray lies on the edge and within the forward's bar of the brute-force model's road range;
    only the model's threshold-sensitive rays are excepted, under the forward's cap"""
    failures, excepted, total = [], [], 0
    for b, w in enumerate(which):
        verts, faces = raw[w]
        m = rm.range_scan(verts, faces, s['boxes'][b], s['sc'][b], s['present'][b], s['ray_sc'][b], max_range, gap, with_agents=False, sensitivity=True)
        sensitive = m['road_lo'] != m['road_hi']
        A, R = out['hit'].shape[1:]
        for a, k in zip(*np.nonzero(np.isfinite(out['road_edge'][b]).all(-1))):
            total += 1
            xi, yi, xj, yj = out['road_edge'][b, a, k].astype(np.float64)
            assert (xi, yi) <= (xj, yj), 'the edge is oriented'
            ox, oy = s['boxes'][b, a, :2].astype(np.float64)
            dy, dx = s['ray_sc'][b, a, k].astype(np.float64)
            wi, wj = dx * (yi - oy) - dy * (xi - ox), dx * (yj - oy) - dy * (xj - ox)
            ui, uj = dx * (xi - ox) + dy * (yi - oy), dx * (xj - ox) + dy * (yj - oy)
            lam = wi / (wi - wj)
            t = ui + (uj - ui) * lam
            slack = GPU_BAR / max(math.hypot(xj - xi, yj - yi), 1e-9)
            if not (-slack <= lam <= 1 + slack and abs(t - m['road'][a, k]) <= GPU_BAR):
                (excepted if sensitive[a, k] else failures).append(f'{label} scene {b} agent {a} ray {k}: edge crossing {t!r} (lambda {lam!r}), model {m["road"][a, k]!r}')
    print(f'{label}: {total} edges, {len(failures)} off the model\'s road range, {len(excepted)} excepted as threshold-sensitive')
    assert not failures, '\n'.join(failures[:20])
    assert len(excepted) <= EXCEPTION_SHARE * out['hit'].size, '\n'.join(excepted[:20])


def sim_case(sim, R, fov):
    from torchdrivesim_amd.infractions import _static_maps_for
    boxes, sc, present, ray_sc = model_inputs(sim, R, fov)
    smap = _static_maps_for(sim.road_mesh, torch.device(DEV)) if sim.road_mesh.faces_count > 0 else None
    return smap, dict(boxes=boxes, sc=sc, present=present, ray_sc=ray_sc)


# ------------------------------------------------------------------------------------------------------------------------ the bar
@pytest.fixture(scope='module')
def town01_sim(towns):
    """Town01, 2 scenes x (12 agents + 4 NPCs) placed by heuristic_initialize_batch"""
    return make_sim(towns, [0, 0], 12, seed=23, npc=4)


@pytest.mark.parametrize('R', [1, 16, 64, 100, 300])
def test_town01(town01_sim, towns, R):
    """R = 1 and 16: a wave holds the rays of several agents; 100: an agent's rays straddle waves; 300: they straddle chunks"""
    smap, s = sim_case(town01_sim, R, 2 * math.pi)
    out = run(smap, s, 50.0, seed=R)
    hold(f'town01 R={R}', s, out, 50.0, least_agent=R // 16, least_road=6 * R)
    edges_end_the_models_road(f'town01 R={R}', out, s, towns[2], [0, 0], 50.0)


def test_a_narrow_field_of_view_and_a_short_range(town01_sim, towns):
    smap, s = sim_case(town01_sim, 64, math.pi / 2)
    out = run(smap, s, 50.0, seed=3)
    hold('town01 fov pi/2', s, out, 50.0, least_road=300)
    out = run(smap, s, 5.0, seed=4)
    live_a, live_r = hold('town01 max_range 5', s, out, 5.0, least_road=10)
    assert (out['road'] == 5.0).mean() > 0.5, 'most rays are capped'
    edges_end_the_models_road('town01 max_range 5', out, s, towns[2], [0, 0], 5.0)


def test_a_batch_on_two_maps_equals_the_single_map_runs(towns):
    from torchdrivesim_amd import _ops
    which = [0, 1, 1, 0]
    sim = make_sim(towns, which, 12, seed=31, npc=4)
    smap, s = sim_case(sim, 64, 2 * math.pi)
    assert isinstance(smap, _ops.StaticMapSet)
    whole = run(smap, s, 50.0, seed=7)
    hold('town01 / town02 multi', s, whole, 50.0, least_agent=4, least_road=1000)
    edges_end_the_models_road('town01 / town02 multi', whole, s, towns[2], which, 50.0)
    g = (torch.from_numpy(whole['g_agent']).to(DEV), torch.from_numpy(whole['g_road']).to(DEV))
    for w in (0, 1):
        idx = [b for b in range(len(which)) if which[b] == w]
        alone, _ = sim_case(make_sim(towns, [w], 12, seed=31, npc=4), 64, 2 * math.pi)      # the town's own mesh, not padded: another grid
        assert isinstance(alone, _ops.StaticMap)
        part = run(alone, {key: v[idx] for key, v in s.items()}, 50.0, g=(g[0][idx], g[1][idx]))
        for key in TENSORS + ('choice', 'road_edge'):
            assert np.array_equal(part[key].view(np.int32), whole[key][idx].view(np.int32)), (w, key)


def test_hand_placed_and_the_parts_alone(towns):
    """outside the grid, off the road, inside each other, an absent agent and an absent NPC; then road=False / agents=False: the skipped
    part's inputs get exact zeros"""
    sim = make_sim(towns, [0, 0], 16, seed=5, npc=4, edit=hand_placed)
    smap, s = sim_case(sim, 64, 2 * math.pi)
    out = run(smap, s, 50.0, seed=12)
    live_a, live_r = hold('town01 hand-placed', s, out, 50.0, least_agent=20, least_road=1000)
    edges_end_the_models_road('town01 hand-placed', out, s, towns[2], [0, 0], 50.0)
    assert not live_r[0, :3].any() and not live_a[0, 4].any() and not live_a[1, 0].any(), 'off the road; inside another rectangle'
    assert not out['g_ray_sc'][1, 3].any() and not out['g_boxes'][1, [3, 18]].any() and not out['g_sc'][1, [3, 18]].any(), 'absent'
    assert (out['choice'][1, 0, :, 0] == 1).all() and (out['choice'][1, 0, :, 1] == 0).all(), 'from inside: the entity, no slab'
    no_road = run(None, s, 50.0, seed=12)
    la, lr = hold('town01 hand-placed road=False', s, no_road, 50.0, least_agent=20, has_road=False)
    assert not lr.any() and np.isnan(no_road['road_edge']).all() and np.array_equal(la, live_a)
    no_agents = run(smap, s, 50.0, want_agents=False, seed=12)
    la, lr = hold('town01 hand-placed agents=False', s, no_agents, 50.0, least_road=1000, want_agents=False)
    assert not la.any() and np.array_equal(lr, live_r) and not no_agents['g_sc'].any() and not no_agents['g_boxes'][..., 2:].any()
    assert not no_agents['g_boxes'][:, 16:].any(), 'NPCs observe nothing'
    # the two parts add up: float64 sums of disjoint terms, rounded once -- compare in float64 against the model of the full run instead of bits
    for key in TENSORS:
        assert np.abs(out[key].astype(np.float64) - no_road[key].astype(np.float64) - no_agents[key].astype(np.float64)).max() <= \
            1e-6 * max(1.0, np.abs(out[key]).max()), key


def test_no_road_mesh(towns):
    sim = make_sim(towns, [0, 0, 0], 16, seed=6, npc=2, road=False)
    smap, s = sim_case(sim, 16, 2 * math.pi)
    assert smap is None
    out = run(smap, s, 40.0, seed=2)
    hold('no road mesh', s, out, 40.0, least_agent=3, has_road=False)
    assert (out['road'] == 40.0).all()


@pytest.mark.parametrize('E', [1, 33, 65, 1024])
def test_synthetic_boxes(E):
    """no map; one entity (nothing to meet), one more than half a wave, one more than a wave, the entity limit (dynamic LDS beyond 64 KiB)"""
    A, R = min(2, E), 16
    s = gm.random_boxes(100 + E, 2, A, E, spread=4.0 * math.sqrt(E))
    s['present'][:, :A] = True
    s['ray_sc'] = gm.rays_of(s['boxes'], A, R)
    out = run(None, s, 100.0, seed=E)
    live_a, _ = hold(f'synthetic E={E}', s, out, 100.0, least_agent=0 if E == 1 else 8, has_road=False)
    if E == 1:
        assert not live_a.any() and all(not out[key].any() for key in TENSORS)
    if E == 1024:
        assert (out['choice'][..., 0] >= 256).any(), 'an entity beyond the first turn of the receiving lanes is met'


def test_identical_boxes_the_lowest_index_receives_everything():
    same = [10.0, 0.5, 4.6, 1.9, 0.4]
    boxes = np.array([[[0.0, 0.0, 4.0, 2.0, 0.1], same, same, same, [-10.0, 3.0, 4.0, 2.0, 2.0]]], np.float32)
    s = dict(boxes=boxes, sc=np.stack([np.sin(boxes[..., 4]), np.cos(boxes[..., 4])], -1).astype(np.float32), present=np.ones((1, 5), bool))
    s['ray_sc'] = gm.rays_of(boxes, 1, 64)
    out = run(None, s, 50.0, seed=1)
    live_a, _ = hold('identical boxes', s, out, 50.0, least_agent=4, has_road=False)
    on_them = (out['choice'][0, 0, :, 0] >= 1) & (out['choice'][0, 0, :, 0] <= 3)
    assert on_them.any() and (out['choice'][0, 0, on_them, 0] == 1).all()
    assert np.abs(out['g_boxes'][0, 1]).max() > 0 and not out['g_boxes'][0, 2:4].any() and not out['g_sc'][0, 2:4].any()


# ------------------------------------------------------------------------------------------------------------------------ exact properties
def test_nan_at_dead_rays_two_runs_and_single_leaves(town01_sim):
    smap, s = sim_case(town01_sim, 64, 2 * math.pi)
    first, again = run(smap, s, 50.0, seed=9), run(smap, s, 50.0, seed=9)
    for key in TENSORS:
        assert np.array_equal(first[key].view(np.int32), again[key].view(np.int32)) and np.abs(first[key]).max() > 0, key
    live_a, live_r = hold('town01 R=64 again', s, first, 50.0)
    ga, gr = first['g_agent'].copy(), first['g_road'].copy()
    assert (~live_a).sum() >= 50 and (~live_r).sum() >= 50
    ga[~live_a], gr[~live_r] = np.nan, np.inf
    ga.flat[np.flatnonzero(~live_a)[::2]] = -np.inf
    gr.flat[np.flatnonzero(~live_r)[::2]] = np.nan
    poisoned = run(smap, s, 50.0, g=(torch.from_numpy(ga).to(DEV), torch.from_numpy(gr).to(DEV)))
    for key in TENSORS:
        assert np.array_equal(first[key].view(np.int32), poisoned[key].view(np.int32)) and np.isfinite(poisoned[key]).all(), key
    for leaf in ('boxes', 'sc', 'ray_sc'):
        only = run(smap, s, 50.0, seed=9, need=(leaf,))
        for key in TENSORS:
            assert (only[key] is None) == (key != 'g_' + leaf), (leaf, key)
        assert np.array_equal(only['g_' + leaf].view(np.int32), first['g_' + leaf].view(np.int32)), leaf
