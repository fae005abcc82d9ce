"""The lane-observation kernel (K8, csrc/lane_obs.hip) on the device against the float64 model of its definition (tests/lane_obs_model.py):
features, points, n_valid and index BIT FOR BIT, no row excepted -- on the synthetic maps of tests/lane_obs_cases.py with the definition's cases,
on the Lanelet2 example map, on Town01 with poses on and off the road, on a ring of 70 lanelets (the selection with its keys in LDS); against
tds_lane_snap; through Simulator.compute_lanes and its batch plumbing over a set of maps; and captured into a graph."""
import math
import os

import numpy as np
import pytest
import torch

import lane_obs_cases as cases
import lane_obs_model as lom
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF = float('inf')
#: (k, n_points, spacing, max_distance): K 1 / 6 / 32 x P 1 / 8 / 32 x spacing 1 / 4 x max_distance 10 / 30 / inf, the defaults among them
COMBOS = [(k, p, spacing, md) for k in (1, 6, 32) for p in (1, 8, 32) for spacing in (1.0, 4.0) for md in (10.0, 30.0, INF)]
NAMES = ('features', 'points', 'n_valid', 'index')


def make_sim(lanelet_maps, states, present=None):
    """a Simulator on an empty road mesh whose scenes have the given lanelet maps (entries may be None); states (B, A, 4) [x, y, psi, speed]"""
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    states = torch.as_tensor(np.asarray(states, np.float32) if not isinstance(states, torch.Tensor) else states).to(DEV).to(torch.float32)
    B, A = states.shape[:2]
    present = torch.ones((B, A), dtype=torch.bool, device=DEV) if present is None else torch.as_tensor(present).to(DEV)
    km = KinematicBicycle()
    km.set_params(lr=torch.full((B, A), 1.9, device=DEV))
    km.set_state(states.contiguous())
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    size = torch.tensor([4.9, 2.0], device=DEV).expand(B, A, 2).contiguous()
    return Simulator(BirdviewMesh.empty(batch_size=B).to(DEV), km, size, present.contiguous(), cfg, renderer=renderer,
                     lanelet_map=None if lanelet_maps is None else list(lanelet_maps))


def as_numpy(obs):
    return tuple(getattr(obs, n).cpu().numpy() for n in NAMES)


def assert_bits(got, want, what):
    """the integers equal, the floats equal as bit patterns (so that -0.0 and 0.0 differ)"""
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert not len(bad), f'{what}: {name} differs at {bad[:8].tolist()}: kernel {g[tuple(bad[0])]!r}, model {w[tuple(bad[0])]!r}'


class Model:
    """the model of a simulator's scenes: the tables once per distinct map, the feet once per observer, whatever the parameters"""
    _tables = {}

    def __init__(self, sim):
        maps = sim.lanelet_map or [None] * sim.batch_size
        for m in maps:
            if m is not None and id(m) not in Model._tables:
                Model._tables[id(m)] = (m, lom.Lanes(m))
        self.lanes = [None if m is None else Model._tables[id(m)][1] for m in maps]
        A = sim.agent_count
        self.xy = sim.get_state()[..., :2].cpu().numpy()
        self.sc = sim._heading_sc()[:, :A].cpu().numpy()              # exactly what compute_lanes hands to the kernel
        self.present = sim.get_present_mask().cpu().numpy()
        self.found = {}

    def __call__(self, k, p, spacing, md):
        return lom.observe_batch(self.lanes, self.xy, self.sc, self.present, k, p, spacing, md, found=self.found)


def check_all_combos(sim, what, combos=COMBOS):
    model = Model(sim)
    filled = points = 0
    for k, p, spacing, md in combos:
        got = as_numpy(sim.compute_lanes(k=k, n_points=p, spacing=spacing, max_distance=md))
        want = model(k, p, spacing, md)
        assert_bits(got, want, f'{what} k={k} n_points={p} spacing={spacing} max_distance={md}')
        filled, points = filled + int((want[3] >= 0).sum()), points + int(want[2].sum())
    assert filled > 0 and points > filled
    return model


# ---------------------------------------------------------------------------------------------------------------- bit equality with the model
@pytest.fixture(scope='module')
def synthetic():
    return {name: make() for name, make in cases.STRUCTURES.items()}


@pytest.mark.parametrize('group', [('edge', 'chain', 'fork', None), ('dead_end', 'loop', 'tagged')])
def test_the_synthetic_maps_with_the_definition_cases(synthetic, group):
    """every scene is seen from the hand-made poses of the definition's cases (the range's closed end and one step beyond, the exact tie at a
    shared end point, polylines that stop at a fork / continue / run into the hop limit, NaN poses) and from random ones: A = 16, one observer
    absent; one scene has no map"""
    rng = np.random.default_rng(len(group))
    maps = [None if g is None else synthetic[g] for g in group]
    states = np.zeros((len(maps), len(cases.HAND_POSES) + 4, 4), np.float32)
    for b, m in enumerate(maps):
        states[b, :len(cases.HAND_POSES), :3] = cases.HAND_POSES
        states[b, len(cases.HAND_POSES):, :3] = cases.poses(rng, m if m is not None else synthetic['chain'], 4)
    present = np.ones(states.shape[:2], bool)
    present[0, 13] = present[1, 2] = False
    sim = make_sim(maps, states, present)
    model = check_all_combos(sim, str(group))
    want = model(4, 8, 4.0, 10.0)
    if None in group:
        assert (want[3][3] == -1).all()                                                  # the scene without a map
        chain = group.index('chain')
        assert want[3][chain, 1].tolist() == [0, 1, -1, -1]                              # the exact tie: the lower index first
        assert want[3][chain, 7, 0] >= 0 and (want[3][chain, 8] == -1).all()             # d2 == r2, and one float32 step of the pose beyond
        assert (want[3][group.index('edge'), 9] == -1).all() and want[3][group.index('edge'), 7, 0] == 0     # one float64 step beyond r2
        assert want[2][group.index('fork'), 2, 0] == 3                                   # the polyline of lanelet 0 stops at the fork
    # every output is written in full: the same call through the entry point into tensors that held something else
    from torchdrivesim_amd import _native as nat, _ops
    B, A = states.shape[:2]
    out = (torch.full((B, A, 4, 8), math.nan, device=DEV), torch.full((B, A, 4, 8, 2), math.nan, device=DEV),
           torch.full((B, A, 4), 99, dtype=torch.int32, device=DEV), torch.full((B, A, 4), 99, dtype=torch.int32, device=DEV))
    lane_set = sim._lane_tables(torch.device(DEV))
    nat.call('tds_lane_observations_multi', torch.device(DEV), lane_set.handle, lane_set.scene_map, sim.get_state()[..., :2].contiguous(),
             sim._heading_sc()[:, :A].contiguous(), _ops._u8(sim.get_present_mask()), *out, B, A, 4, 8, 4.0, 10.0)
    assert_bits(tuple(t.cpu().numpy() for t in out), want, 'into used tensors')


def test_the_lanelet2_example_map():
    from torchdrivesim_amd import lanelet2
    m = lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'testing_lanelet2map.osm'), origin=(0.0, 0.0))
    rng = np.random.default_rng(5)
    states = np.zeros((2, 6, 4), np.float32)
    states[..., :3] = cases.poses(rng, m, 12, spread=4.0).reshape(2, 6, 3)
    check_all_combos(make_sim([m, m], states), 'testing_lanelet2map')


@pytest.fixture(scope='module')
def towns():
    from torchdrivesim_amd import lanelet2
    return {k: lanelet2.load_lanelet_map(os.path.join(GOLDEN, f), origin=(0.0, 0.0)) for k, f in (('Town01', 'carla_Town01.osm.gz'),
                                                                                                 ('Town02', 'carla_Town02.osm.gz'))}


def town_states(maps, A, seed):
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    _, states, placed = heuristic_initialize_batch(list(maps), len(maps), A, seed=seed, device=DEV)
    assert bool(placed.all())
    return states.clone()


def test_town01_on_and_off_the_road(towns):
    """B = 2, A = 8 from heuristic_initialize_batch; in each scene three agents are moved 5 .. 40 m off the road, one is absent"""
    m = towns['Town01']
    states = town_states([m, m], 8, seed=11)
    g = torch.Generator().manual_seed(12)
    angle, dist = torch.rand(2, 3, generator=g) * 2 * math.pi, 5.0 + 35.0 * torch.rand(2, 3, generator=g)
    states[:, 5:, 0] += (dist * torch.cos(angle)).to(DEV)
    states[:, 5:, 1] += (dist * torch.sin(angle)).to(DEV)
    present = np.ones((2, 8), bool)
    present[1, 3] = False
    check_all_combos(make_sim([m, m], states, present), 'Town01')


def test_more_than_64_lanelets_select_with_their_keys_in_lds():
    """a ring of 70 short lanelets (L > 64: tds::select_by_rounds), beside a scene of three (L <= 64: by rank) in the same launch"""
    ring, chain = cases.ring(70), cases.chain()
    rng = np.random.default_rng(70)
    states = np.zeros((3, 6, 4), np.float32)
    states[0, :, :3], states[1, :, :3], states[2, :, :3] = cases.poses(rng, ring, 6), cases.poses(rng, chain, 6), cases.poses(rng, ring, 6, spread=1.0)
    states[2, 0, :3] = [0.0, 0.0, 1.0]                                                    # the centre: 70 distances that agree to rounding
    model = check_all_combos(make_sim([ring, chain, ring], states), 'ring of 70')
    assert (model(32, 8, 4.0, INF)[3][0] >= 64).any()                                     # winners beyond the first 64 lanelets


def test_refusals():
    from torchdrivesim_amd import _native as nat, _ops
    big = cases.make_map([cases.lanelet(i, [(3.0 * i, 0.0), (3.0 * i + 2.0, 0.0)], 2 * i, 2 * i + 1) for i in range(2049)])
    states = np.zeros((1, 2, 4), np.float32)
    with pytest.raises(nat.TdsError, match='2049 lanelets') as err:
        make_sim([big], states).compute_lanes()
    assert err.value.code == nat.E_LIMIT
    sim = make_sim([cases.chain(), cases.fork()], np.zeros((2, 2, 4), np.float32))
    lane_set = sim._lane_tables(torch.device(DEV))
    xy, sc, pres = sim.get_state()[..., :2].contiguous(), sim._heading_sc().contiguous(), _ops._u8(sim.get_present_mask())
    out = lambda k=4, p=8: (torch.zeros((2, 2, k, 8), device=DEV), torch.zeros((2, 2, k, p, 2), device=DEV),
                            torch.zeros((2, 2, k), dtype=torch.int32, device=DEV), torch.zeros((2, 2, k), dtype=torch.int32, device=DEV))
    call = lambda k, p, spacing, md, smap=lane_set.scene_map, B=2: nat.call('tds_lane_observations_multi', torch.device(DEV), lane_set.handle, smap, xy, sc,
                                                                           pres, *out(max(k, 1), max(p, 1)), B, 2, k, p, spacing, md)
    call(4, 8, 4.0, 30.0)
    for bad in [(0, 8, 4.0, 30.0), (33, 8, 4.0, 30.0), (4, 0, 4.0, 30.0), (4, 33, 4.0, 30.0), (4, 8, 0.0, 30.0), (4, 8, -1.0, 30.0), (4, 8, INF, 30.0),
                (4, 8, math.nan, 30.0), (4, 8, 4.0, -1.0), (4, 8, 4.0, math.nan)]:
        with pytest.raises(nat.TdsError) as err:
            call(*bad)
        assert err.value.code == nat.E_INVAL, bad
    with pytest.raises(nat.TdsError, match='needs scene_map') as err:                     # a set of two tables without scene_map
        call(4, 8, 4.0, 30.0, smap=None)
    assert err.value.code == nat.E_INVAL
    call(4, 8, 4.0, 30.0, B=0)                                                            # B * A == 0: a successful no-op
    for bad in [dict(k=0), dict(k=33), dict(n_points=0), dict(n_points=33), dict(spacing=0.0), dict(spacing=math.nan), dict(max_distance=-1.0)]:
        with pytest.raises(ValueError, match='lanes: '):
            sim.compute_lanes(**bad)


# ---------------------------------------------------------------------------------------------------------------- agreement with tds_lane_snap
def test_arc_and_lateral_are_those_of_snap_to_lanes(towns):
    """for poses on a lane, the slot whose index is the lane snap_to_lanes finds has arc == float32(snap's arc) and snap's lateral, bit for bit"""
    from torchdrivesim_amd.lanelet2 import snap_to_lanes
    m = towns['Town01']
    states = town_states([m, m, m], 8, seed=23)
    lane, arc, lateral = snap_to_lanes([m, m, m], states, tolerance=1.0)
    obs = make_sim([m, m, m], states).compute_lanes(k=32, n_points=1, max_distance=10.0)
    on = lane >= 0
    assert int(on.sum()) >= 20                                                            # (of 24: placed on a lane, along it)
    hit = (obs.index == lane.unsqueeze(-1)) & on.unsqueeze(-1)
    assert bool((hit.sum(-1) == on.to(torch.int64)).all())                                # the lane is one of the slots, once
    assert torch.equal(obs.features[..., 4][hit].view(torch.int32), arc[on].to(torch.float32).view(torch.int32))
    assert torch.equal(obs.features[..., 6][hit].view(torch.int32), lateral[on].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- batch plumbing
def equal(a, b):
    return all(torch.equal(getattr(a, n).view(torch.int32), getattr(b, n).view(torch.int32)) for n in NAMES)


def rows(obs, idx):
    from torchdrivesim_amd.simulator import Lanes
    return Lanes(*(getattr(obs, n)[idx] for n in NAMES))


@pytest.fixture(scope='module')
def mixed(towns):
    """B = 4: Town01 / Town02 / no map / Town01, A = 4"""
    t1, t2 = towns['Town01'], towns['Town02']
    return make_sim([t1, t2, None, t1], town_states([t1, t2, t1, t1], 4, seed=31))


def test_a_set_of_maps_and_the_batch_plumbing(mixed):
    from torchdrivesim_amd.parallel import shard_simulator
    from torchdrivesim_amd.simulator import Lanes
    kw = dict(k=5, n_points=6, spacing=4.0, max_distance=25.0)
    whole = mixed.compute_lanes(**kw)
    assert isinstance(whole, Lanes) and whole.features.shape == (4, 4, 5, 8) and whole.points.shape == (4, 4, 5, 6, 2) and not whole.features.requires_grad
    assert whole.n_valid.dtype == whole.index.dtype == torch.int32 and Lanes.FEATURES[4] == 'arc' and len(Lanes.FEATURES) == 8
    assert_bits(as_numpy(whole), Model(mixed)(5, 6, 4.0, 25.0), 'Town01 / Town02 / None / Town01')
    assert bool((whole.index[2] == -1).all()) and not bool(whole.features[2].any()) and bool(whole.mask[[0, 1, 3]].any(-1).all())
    assert torch.equal(whole.mask, whole.index >= 0)
    assert torch.equal(whole.points_mask, torch.arange(6, device=DEV) < whole.n_valid[..., None]) and not bool(whole.points[~whole.points_mask].any())
    assert equal(mixed.compute_lanes(**kw), whole) and equal(mixed.copy().compute_lanes(**kw), whole)          # repeated calls, a copy
    idx = [3, 1]
    assert equal(mixed.select_batch_elements(idx, in_place=False).compute_lanes(**kw), rows(whole, idx))
    assert equal(mixed[[2]].compute_lanes(**kw), rows(whole, [2])) and equal(mixed[[1, 2]].compute_lanes(**kw), rows(whole, [1, 2]))
    assert equal(mixed.extend(2, in_place=False).compute_lanes(**kw), rows(whole, [0, 0, 1, 1, 2, 2, 3, 3]))
    shards = [shard_simulator(mixed, rank, 2).compute_lanes(**kw) for rank in range(2)]
    assert equal(Lanes(*(torch.cat([getattr(s, n) for s in shards]) for n in NAMES)), whole)
    assert_bits(as_numpy(mixed.compute_lanes()), Model(mixed)(6, 8, 4.0, 30.0), 'the defaults')


def test_no_lanelet_map_and_no_agents(towns):
    states = np.zeros((2, 3, 4), np.float32)
    for maps in (None, [None, None]):
        obs = make_sim(maps, states).compute_lanes(k=3, n_points=5)
        assert obs.features.shape == (2, 3, 3, 8) and obs.points.shape == (2, 3, 3, 5, 2) and obs.n_valid.shape == obs.index.shape == (2, 3, 3)
        assert not bool(obs.features.any()) and not bool(obs.points.any()) and not bool(obs.n_valid.any()) and bool((obs.index == -1).all())
        assert not bool(obs.mask.any()) and not bool(obs.points_mask.any())
    from torchdrivesim_amd import _ops
    lane_set = make_sim([towns['Town01']] * 2, states)._lane_tables(torch.device(DEV))
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    out = _ops.lane_observations(lane_set, z(2, 0, 2), z(2, 0, 2), z(2, 0, dtype=torch.bool), 6, 8, 4.0, 30.0)             # no exposed agents
    assert [tuple(t.shape) for t in out] == [(2, 0, 6, 8), (2, 0, 6, 8, 2), (2, 0, 6), (2, 0, 6)]


def test_a_captured_step_and_lanes_replays_the_eager_bits(towns):
    """step + compute_lanes captured on one stream into a graph, warmed up eagerly first (the lane tables are built then); three replays equal eager"""
    m = towns['Town01']
    start = town_states([m] * 3, 6, seed=41)
    live, ref = make_sim([m] * 3, start), make_sim([m] * 3, start)
    B, A = 3, 6
    g0 = torch.Generator(device='cpu').manual_seed(3)
    actions = (torch.rand(3, B, A, 2, generator=g0) * 2 - 1).to(DEV)
    state = live.get_state().clone()
    action = actions[0].clone()

    def step():
        live.kinematic_model.set_state(state)
        live.step(action)
        return live.compute_lanes(), live.get_state()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        obs, new = step()
        state_next = new.clone()
    for i in range(3):
        ref.kinematic_model.set_state(state.clone())
        ref.step(actions[i])
        want = ref.compute_lanes()
        action.copy_(actions[i])
        g.replay()
        torch.cuda.synchronize()
        assert equal(obs, want) and torch.equal(new, ref.get_state())
        assert bool(obs.mask.any())
        state.copy_(state_next)
