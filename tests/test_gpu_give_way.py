"""Giving way at junctions on the device (csrc/conflicts.hip `tds_lane_conflicts_f64`, `tds_lane_give_way_multi`; csrc/follow.hip
`tds_lane_follow_step_stops_multi`; behavior/lane_follow.py `give_way=True`) against the float64 model of its definition (tests/give_way_model.py).

The bar: the conflict tables equal BIT FOR BIT; `stop_at`, `yield_to`, `lane`, `hops`, `leader` equal; `arc`, `speed`, `x`, `y`, `[sin, cos]` equal bit for
bit; `psi`, a float64 atan2 rounded once, within one float32 ulp (the bar of tests/test_gpu_lane_follow.py).  No row is excepted."""
import ctypes
import os

import numpy as np
import pytest
import torch

import give_way_cases as gc
import give_way_model as gw
import lane_follow_model as lf
import test_gpu_lane_follow as base
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
KEYS = ('lane', 'arc', 'hops', 'leader', 'npc_state', 'npc_sc', 'npc_present_mask', 'stop_at', 'yield_to')


@pytest.fixture(scope='module')
def world():
    """name -> (map, model, the model's conflict tables); computed once, never changed"""
    from torchdrivesim_amd import lanelet2
    maps = {f'Town0{k}': lanelet2.load_lanelet_map(os.path.join(GOLDEN, f'carla_Town0{k}.osm.gz'), origin=(0.0, 0.0)) for k in (1, 2)}
    maps['crossing'] = gc.crossing_map()
    out = {}
    for name, m in maps.items():
        model = lf.Lanes(m)
        out[name] = (m, model, gw.conflict_tables(model))
    return out


def device_tables(lanelet_map, clearance=2.0, step=0.5):
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import LANELET_TAGS_TO_EXCLUDE
    table = lanelet_map.table(torch.device(DEV), LANELET_TAGS_TO_EXCLUDE)
    return table, [t.cpu().numpy() for t in _ops.lane_conflicts(table, clearance, step)[:3]]


def assert_tables_equal(got, want, tag):
    for g, w, what in zip(got, want, ('exit', 'zone_in', 'zone_out')):
        assert g.shape == w.shape and np.array_equal(g, w), (tag, what, np.argwhere(g != w)[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------- conflict tables
def with_a_lanelet_nothing_can_drive_on():
    """the crossing, and in the middle of it a lanelet whose bounds are one point each: its centre line has no length"""
    from torchdrivesim_amd import lanelet2
    m = gc.crossing_map()
    spot = np.array([[0.5, 0.5, 0.0], [0.5, 0.5, 0.0]])
    return lanelet2.LaneletMap([], np.zeros((0, 3)), m.laneletLayer + [lanelet2.Lanelet(99, spot, spot + 0.25, np.array([900, 902]), np.array([901, 903]), {'type': 'lanelet'})])


@pytest.mark.parametrize('name', ['Town01', 'Town01 reverted', 'Town02', 'Town02 reverted', 'testing', 'crossing', 'one lanelet', 'undrivable'])
def test_conflict_tables_equal_the_model(world, name):
    from torchdrivesim_amd import lanelet2
    if name.split()[0] in world:
        m, model, want = world[name.split()[0]]
        if name.endswith('reverted'):
            m = lanelet2.revert_map(m)
            model = lf.Lanes(m)
            want = gw.conflict_tables(model)
    else:
        m = {'testing': lambda: lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'testing_lanelet2map.osm'), origin=(0.0, 0.0)),
             'one lanelet': lambda: base_straight_map(), 'undrivable': with_a_lanelet_nothing_can_drive_on}[name]()
        model = lf.Lanes(m)
        want = gw.conflict_tables(model)
    _, got = device_tables(m)
    assert_tables_equal(got, want, name)
    pairs = int(gw.conflicting(got).sum())
    assert pairs == {'Town01': 144, 'Town02': 96, 'crossing': 8, 'undrivable': 8}.get(name.split()[0], 0)
    if name == 'undrivable':
        assert not model.eligible(12) and (got[0][12] == -1).all() and (got[0][:, 12] == -1).all()


def base_straight_map():
    from test_lane_follow_model import straight_map
    return straight_map(100.0, 1)


def test_conflict_tables_at_another_clearance_and_step(world):
    m, model, _ = world['Town01']
    table, got = device_tables(m, 1.5, 0.25)
    assert_tables_equal(got, gw.conflict_tables(model, 1.5, 0.25), 'Town01 1.5 / 0.25')
    assert int(gw.conflicting(got).sum()) == 144
    from torchdrivesim_amd import _ops
    assert _ops.lane_conflicts(table, 1.5, 0.25)[3] is _ops.lane_conflicts(table, 1.5, 0.25)[3], 'built once per (table, clearance, step)'
    assert _ops.lane_conflicts(table, 2.0, 0.5)[3] is not _ops.lane_conflicts(table, 1.5, 0.25)[3]


def test_table_argument_errors_come_before_any_launch(world):
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import LANELET_TAGS_TO_EXCLUDE
    table = world['crossing'][0].table(torch.device(DEV), LANELET_TAGS_TO_EXCLUDE)
    for clearance, step in ((0.0, 0.5), (2.0, 0.0), (float('nan'), 0.5), (2.0, float('inf')), (-1.0, 0.5)):
        with pytest.raises(nat.TdsError) as e:
            _ops.lane_conflicts(table, clearance, step)
        assert e.value.code == nat.E_INVAL
        rc = nat.lib().tds_lane_conflicts_f64(table.handle, None, clearance, step, None)       # a null table: nothing could have been written
        assert rc == nat.E_INVAL and 'clearance and step' in nat.last_error()
    assert nat.lib().tds_lane_conflicts_f64(None, None, 2.0, 0.5, None) == nat.E_INVAL


# ---------------------------------------------------------------------------------------------------------------- simulators by hand
def make_sim(maps, states, present, A, seed, dt=0.1, lights=None, v0=8.0, **ctrl_kw):
    """B scenes, scene b on maps[b] (None: no lane map); states (B, A + N, 4) and present (B, A + N) placed by hand, the first A rows exposed agents"""
    from torchdrivesim_amd.behavior.lane_follow import LaneFollowingNPCController
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    states, present = torch.as_tensor(np.asarray(states, F32), device=DEV), torch.as_tensor(np.asarray(present, bool), device=DEV)
    B, E = present.shape
    size = torch.tensor(gc.SIZE, device=DEV).expand(B, E, 2).contiguous()
    km = KinematicBicycle(dt=dt)
    km.set_params(lr=torch.full((B, A), 1.5, device=DEV))
    km.set_state(states[:, :A].contiguous())
    ctrl_kw.setdefault('give_way', True)
    ctrl = LaneFollowingNPCController(list(maps), size[:, A:].contiguous(), states[:, A:].contiguous(), present[:, A:].contiguous(), seed=seed,
                                      desired_speed=v0, **ctrl_kw)
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    return Simulator(BirdviewMesh.empty(batch_size=B).to(DEV), km, size[:, :A].contiguous(), present[:, :A].contiguous(), cfg, renderer=renderer,
                     npc_controller=ctrl, lanelet_map=list(maps), traffic_controls=lights)


def snapshot(ctrl):
    return {k: getattr(ctrl, k).clone() for k in KEYS if getattr(ctrl, k) is not None}


def step_and_compare(sim, models, what=''):
    """one Simulator.step, the NPC rows against the model; models[b] = (model, tables) or None; returns the model's per-scene outputs"""
    ctrl = sim.npc_controller
    B, N = ctrl.npc_state.shape[:2]
    A = sim.agent_count
    before = {k: v.cpu().numpy() for k, v in snapshot(ctrl).items()}
    boxes, sc, speed, present = (t.cpu().numpy() for t in ctrl._entities(sim))
    lines = ctrl._stop_lines(sim)
    lines = None if lines is None else [t.cpu().numpy() for t in lines]
    size, v0, ids = ctrl.npc_size.cpu().numpy(), ctrl.desired_speed.cpu().numpy(), ctrl.scene_ids.cpu().numpy()
    sim.step(torch.zeros((B, A, 2), device=DEV))
    after = {k: v.cpu().numpy() for k, v in snapshot(ctrl).items()}
    outs = []
    for b in range(B):
        tag = f'{what} scene {b}'
        got = after['npc_state'][b]
        if models[b] is None:                                               # no lane map: nothing moves, nobody yields
            assert np.array_equal(got, before['npc_state'][b]) and (after['leader'][b] == -1).all() and (after['yield_to'][b] == -1).all()
            assert np.isinf(after['stop_at'][b]).all()
            outs.append(None)
            continue
        model, tables = models[b]
        out = gw.step_scene(model, tables, before['lane'][b], before['arc'][b], before['hops'][b], before['npc_state'][b], size[b], v0[b],
                            before['npc_present_mask'][b], boxes[b], sc[b], speed[b], present[b], np.arange(A, A + N), ctrl.seed, int(ids[b]),
                            sim.kinematic_model.dt, [] if lines is None else list(zip(lines[0][b], lines[1][b], lines[2][b])), ctrl.horizon,
                            ctrl.lateral_margin, ctrl.idm, ctrl.creep_speed)
        outs.append(out)
        for k in ('stop_at', 'yield_to', 'lane', 'hops', 'leader'):
            assert np.array_equal(after[k][b], out[k]), (tag, k, np.nonzero(after[k][b] != out[k])[0], after[k][b], out[k])
        assert np.array_equal(after['arc'][b], out['arc']), (tag, 'arc', np.abs(after['arc'][b] - out['arc']).max())
        want = out['state']
        for c, name in ((0, 'x'), (1, 'y'), (3, 'speed')):
            assert np.array_equal(got[:, c], want[:, c]), (tag, name, np.abs(got[:, c] - want[:, c]).max())
        assert base.within_one_ulp(got[:, 2], want[:, 2]).all(), (tag, 'psi')
        moved = out['moved']
        assert np.array_equal(after['npc_sc'][b][moved], out['sc'][moved]), (tag, '[sin, cos]')
        assert np.array_equal(got[~moved], before['npc_state'][b][~moved]) and (after['leader'][b][~moved] == -1).all()
    return outs


# ---------------------------------------------------------------------------------------------------------------- hand-placed scenes
A2, N12, SEED = 2, 12, 77
FAR = [9000.0, 9000.0, 0.0, 0.0]


def approaches(model, tables, seed, scene_id, rows, merging, used):
    """a pair of conflicting junction lanelets (p, q) -- merging into a common successor, or crossing -- with a predecessor of each from which NPCs
    rows[0] / rows[1] of this scene draw p / q as their successor at hop 0, more than 24 m long; at a junction not yet in `used`"""
    C = gw.conflicting(tables)
    pred = [[a for a in range(len(model)) if l in model.succ[a]] for l in range(len(model))]
    junction = list(range(len(model)))                                      # lanelets that conflict, directly or through others, are one junction
    for _ in range(len(model)):
        junction = [min([junction[a]] + [junction[b] for b in np.nonzero(C[a])[0]]) for a in range(len(model))]
    for p, q in np.argwhere(C).tolist():
        if (model.succ[p] == model.succ[q]) != merging or junction[p] in used:
            continue
        for pp in pred[p]:
            for pq in pred[q]:
                if pp != pq and min(model.length(pp), model.length(pq)) > 24.0 and \
                        model.successor(pp, seed, scene_id, rows[0], 0) == p and model.successor(pq, seed, scene_id, rows[1], 0) == q:
                    used.add(junction[p])
                    return p, q, pp, pq
    raise AssertionError('no such pair on this map')


def hand_placed(world, names, dt=0.1):
    """per scene on a town (NPC n is row A2 + n): NPCs 0 / 1 approach a crossing pair 14 m / 10 m before their lanelets' ends at 6 m/s, NPCs 2 / 3 a merging pair
    likewise; NPC 4 follows 8 m behind NPC 0; NPC 5 is absent; NPC 6 is off the map (lane -1); NPCs 7 / 8 approach a third pair 10 m / 14 m before the
    ends, NPC 7 (the nearer) behind a RED stop line 4 m before its lanelet's end, NPC 8 behind a GREEN one; a third, padded line lies before NPC 0.
    A scene whose name is None has no lane map: its rows stand where they are."""
    B = len(names)
    states, present = np.tile(np.array(FAR, F32), (B, A2 + N12, 1)), np.zeros((B, A2 + N12), bool)
    spots, models = [], []
    for b, name in enumerate(names):
        states[b, :, 0] += 50.0 * np.arange(A2 + N12)
        present[b] = True
        present[b, A2 + 5] = False
        if name is None:
            spots.append([FAR] * 3), models.append(None)
            continue
        _, m, tables = world[name]
        models.append((m, tables))
        used = set()
        cross, merge, third = (approaches(m, tables, SEED, b, rows, merging, used) for rows, merging in (((0, 1), False), ((2, 3), True), ((7, 8), False)))
        put = lambda n, l, back, v: states[b].__setitem__(A2 + n, base.pose_row(m, l, m.length(l) - back, v))
        put(0, cross[2], 14.0, 6.0), put(1, cross[3], 10.0, 6.0), put(4, cross[2], 22.0, 6.0)
        put(2, merge[2], 14.0, 6.0), put(3, merge[3], 10.0, 6.0)
        put(7, third[2], 10.0, 6.0), put(8, third[3], 14.0, 6.0)
        spots.append([base.pose_row(m, third[2], m.length(third[2]) - 4.0, 0.0), base.pose_row(m, third[3], m.length(third[3]) - 4.0, 0.0),
                      base.pose_row(m, cross[2], m.length(cross[2]) - 4.0, 0.0)])
    return states, present, spots, models


def lights_for(spots):
    from torchdrivesim_amd.traffic_controls import TrafficLightControl
    pos = torch.tensor([[[x, y, 0.5, 4.0, psi] for x, y, psi, _ in scene] for scene in spots], dtype=torch.float32, device=DEV)
    mask = torch.tensor([[True, True, False]] * len(spots), device=DEV)
    lights = TrafficLightControl(pos, mask=mask)
    lights.set_state(torch.tensor([[0, 2, 0]] * len(spots), device=DEV))           # red, green, (padding) red
    return {'traffic_light': lights}


NAMES = ['Town01', 'Town02', None, 'Town01', 'Town02']


@pytest.mark.parametrize('dt', [0.1, 2.0])
def test_hand_placed_pairs_equal_the_model(world, dt):
    """scenes alternating Town01 / Town02 and one without a map; crossing and merging pairs, a follower behind a yielding NPC, an absent row, a row off the
    map, red, green and padded stop lines; single steps of 0.1 s, and of 2 s"""
    states, present, spots, models = hand_placed(world, NAMES)
    maps = [None if n is None else world[n][0] for n in NAMES]
    sim = make_sim(maps, states, present, A2, SEED, dt=dt, lights=lights_for(spots))
    ctrl = sim.npc_controller
    assert (ctrl.lane[:, 6] == -1).all() and (ctrl.lane[2] == -1).all()
    for it in range(3 if dt < 1 else 2):
        outs = step_and_compare(sim, models, what=f'dt {dt} step {it}')
        if it:
            continue
        lines = [t.cpu().numpy() for t in ctrl._stop_lines(sim)]
        for b, out in enumerate(outs):
            if out is None:
                continue
            y = out['yield_to']
            for i, j, where in ((0, 1, 'crossing'), (2, 3, 'merge')):       # which of the two: the model says (their zones begin at different arcs)
                assert (y[i], y[j]) in ((j, -1), (-1, i)), f'at the {where} one of the two gives way to the other'
                assert out['leader'][i if y[i] >= 0 else j] == -3
            assert out['leader'][4] in (A2 + 0, -3), 'the follower brakes for the NPC in front of it, or for the junction that one waits at'
            assert y[7] == -1 and y[8] == -1, 'nobody waits for the NPC at the red light, and it waits for its light, not for the junction'
            assert lines[0][b][0] == ctrl.lane[b, 7].item() and lines[2][b].tolist() == [True, False, False]
            assert np.isinf(out['stop_at'][[5, 6]]).all() and (y[[5, 6]] == -1).all()


def behind_an_agent(states):
    """(B, N, 4) NPC states -> (states (B, 1 + N, 4), present): one exposed agent far away in front of them"""
    states = np.concatenate([np.tile(np.array(FAR, F32), (len(states), 1, 1)), states], 1)
    return states, np.ones(states.shape[:2], bool)


def spread(model, n, gap=20.0):
    """n poses [lanelet, arc] along the drivable lanelets in index order, every `gap` metres from 5 m"""
    out = []
    for l in range(len(model)):
        if model.eligible(l) and not model.flag[l]:
            out += [(l, a) for a in np.arange(5.0, model.length(l) - 1.0, gap)]
    assert len(out) >= n
    return out[:n]


@pytest.mark.parametrize('N', [1, 2, 65])
def test_shapes(world, N):
    """one NPC; two (a pair at the synthetic crossing, an exact tie); 65: more than one wave of NPCs, on Town01 and Town02"""
    if N == 2:
        m, model, tables = world['crossing']
        states = np.array([[base.pose_row(model, 0, 40.0, 6.0), base.pose_row(model, 3, 40.0, 6.0)]] * 2, F32)
        sim = make_sim([m, m], *behind_an_agent(states), 1, SEED)
        for it in range(3):
            outs = step_and_compare(sim, [(model, tables)] * 2, what=f'N 2 step {it}')
            assert all(o['yield_to'].tolist() == [-1, 0] for o in outs), 'an exact tie goes to the lower index'
        return
    names = ['Town01', 'Town02']
    states = np.array([[base.pose_row(world[n][1], l, a, 6.0) for l, a in spread(world[n][1], N)] for n in names], F32)
    sim = make_sim([world[n][0] for n in names], *behind_an_agent(states), 1, SEED + N)
    yields = 0
    for it in range(3):
        outs = step_and_compare(sim, [world[n][1:] for n in names], what=f'N {N} step {it}')
        yields += sum(int((o['yield_to'] >= 0).sum()) for o in outs)
    assert N == 1 or yields > 0


# ---------------------------------------------------------------------------------------------------------------- rollouts
def rollout_start(world, B=2, N=32):
    model = world['Town01'][1]
    poses = spread(model, B * N, gap=35.0)
    return np.array([[base.pose_row(model, l, a, 5.0) for l, a in poses[b::B]] for b in range(B)], F32)


def test_a_rollout_of_100_steps_stays_on_the_model(world):
    m, model, tables = world['Town01']
    sim = make_sim([m, m], *behind_an_agent(rollout_start(world)), 1, 211)
    yields = waits = 0
    for it in range(100):
        outs = step_and_compare(sim, [(model, tables)] * 2, what=f'rollout step {it}')
        yields += sum(int((o['yield_to'] >= 0).sum()) for o in outs)
        waits += sum(int((o['leader'] == -3).sum()) for o in outs)
    print('rollout: NPC-steps giving way', yields, 'braking for a junction', waits, 'hops', int(sim.npc_controller.hops.sum()))
    assert yields > 0 and waits > 0 and int(sim.npc_controller.hops.sum()) >= 32


def test_with_the_option_off_the_rollout_is_the_follow_kernel_alone(world):
    """give_way=False: the controller's step is one call of tds_lane_follow_step_multi, as before the option existed -- recorded here by calling
    that entry point on copies of the buffers; and the extended entry point without stops is that kernel bit for bit"""
    from torchdrivesim_amd import _native as nat
    m = world['Town01'][0]
    sim = make_sim([m, m], *behind_an_agent(rollout_start(world)), 1, 211, give_way=False)
    ctrl = sim.npc_controller
    assert ctrl.stop_at is None and ctrl.yield_to is None and ctrl._conflicts is None
    B, N = ctrl.npc_state.shape[:2]
    dev = torch.device(DEV)
    self_index = torch.arange(1, 1 + N, dtype=torch.int32, device=dev).expand(B, N).contiguous()
    idm = (ctypes.c_float * 5)(*ctrl.idm)
    old, ext = snapshot(ctrl), snapshot(ctrl)
    for it in range(100):
        boxes, esc, speed, present = ctrl._entities(sim)
        E = boxes.shape[1]
        for name, mine, extra in (('tds_lane_follow_step_multi', old, ()), ('tds_lane_follow_step_stops_multi', ext, (None,))):
            nat.call(name, dev, ctrl._lane_table_set().handle, ctrl._lane_table_set().scene_map, ctrl.scene_ids, B, N, E, boxes.contiguous(), esc.contiguous(),
                     speed, present.contiguous().view(torch.uint8), self_index, ctrl.npc_size.contiguous(), ctrl.desired_speed,
                     ctrl.npc_present_mask.view(torch.uint8), mine['lane'], mine['arc'], mine['hops'], mine['npc_state'], mine['npc_sc'], mine['leader'],
                     *extra, ctrl.seed, 0.1, ctrl.horizon, ctrl.lateral_margin, ctypes.cast(idm, ctypes.c_void_p))
        sim.step(torch.zeros((B, 1, 2), device=DEV))
        now = snapshot(ctrl)
        assert base.same(now, old) and base.same(now, ext), f'step {it}'
    assert int(ctrl.hops.sum()) >= 32 and not bool((ctrl.leader == -3).any())


# ---------------------------------------------------------------------------------------------------------------- batch plumbing
def test_batch_operations_reproduce_the_rows_bit_for_bit(world):
    from torchdrivesim_amd.behavior.lane_follow import LaneFollowingNPCController
    from torchdrivesim_amd.parallel import shard_simulator
    names = ['Town01', 'Town02', 'Town02', 'Town01', 'Town01', 'Town02']
    B, steps = len(names), 6
    states, present, spots, _ = hand_placed(world, names)
    maps = [world[n][0] for n in names]
    build = lambda: make_sim(maps, states, present, A2, SEED, lights=lights_for(spots))
    sim = build()
    idx = [4, 0, 3]
    variants = {'select': (sim.select_batch_elements(idx, in_place=False), idx), 'copy': (sim.copy(), list(range(B))),
                'extend': (sim.extend(2, in_place=False), [b for b in range(B) for _ in range(2)]),
                'shard 0': (shard_simulator(sim, 0, 2), [0, 1, 2]), 'shard 1': (shard_simulator(sim, 1, 2), [3, 4, 5])}
    alone = build().select_batch_elements([2, 5], in_place=False)
    c = alone.npc_controller
    assert torch.equal(c.scene_ids, torch.tensor([2, 5], device=DEV)) and c.give_way and c.stop_at.shape == (2, N12)
    alone.npc_controller = LaneFollowingNPCController([c.lanelet_maps[0], c.lanelet_maps[1]], c.npc_size, c.npc_state, c.npc_present_mask, seed=c.seed,
                                                      scene_ids=torch.tensor([2, 5], device=DEV), give_way=True)
    variants['explicit scene_ids'] = (alone, [2, 5])
    zero = torch.zeros((B, A2, 2), device=DEV)
    for t in range(steps):
        sim.step(zero)
        for other, rows in variants.values():
            other.step(zero[rows])
    whole = snapshot(sim.npc_controller)
    assert bool((whole['yield_to'] >= 0).any()) and bool((whole['leader'] == -3).any())
    for name, (other, rows) in variants.items():
        part = snapshot(other.npc_controller)
        for k in whole:
            assert torch.equal(part[k], whole[k][rows]), (name, k)
    before = snapshot(sim.npc_controller)
    variants['copy'][0].step(zero)
    assert base.same(snapshot(sim.npc_controller), before), 'the copy shares no buffer with the original'
    # what the last step decided goes with a copy, a selection and an extension before they are stepped
    for other, rows in ((sim.copy(), list(range(B))), (sim.select_batch_elements(idx, in_place=False), idx), (sim.extend(2, in_place=False), variants['extend'][1])):
        part = snapshot(other.npc_controller)
        assert all(torch.equal(part[k], before[k][rows]) for k in before) and part['stop_at'].data_ptr() != before['stop_at'].data_ptr()


# ---------------------------------------------------------------------------------------------------------------- graph capture
def test_a_captured_step_replays_the_eager_bits(world):
    names = ['Town01', 'Town02'] * 2
    states, present, spots, _ = hand_placed(world, names)
    maps = [world[n][0] for n in names]
    sim, ref = (make_sim(maps, states, present, A2, SEED, lights=lights_for(spots)) for _ in range(2))
    B = len(names)
    state = sim.get_state().clone()
    action = torch.zeros((B, A2, 2), device=DEV)
    ctrl = sim.npc_controller
    start = snapshot(ctrl)

    def step():
        sim.kinematic_model.set_state(state)
        sim.step(action)
        return sim.get_state()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()                                          # warm-up: lane and conflict tables, the self-index rows, the stop lines' lanes
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k, v in start.items():
        getattr(ctrl, k).copy_(v)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        new = step()
        state_next = new.clone()
    for k, v in start.items():
        getattr(ctrl, k).copy_(v)
    for i in range(10):
        ref.step(action)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(new, ref.get_state()) and base.same(snapshot(ctrl), snapshot(ref.npc_controller)), f'replay {i}'
        state.copy_(state_next)
    assert bool((ctrl.arc != start['arc']).any()) and bool((ctrl.yield_to >= 0).any())


# ---------------------------------------------------------------------------------------------------------------- limits
def test_more_npcs_than_a_workgroup_are_refused_before_any_launch(world):
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.behavior.lane_follow import LaneFollowingNPCController
    m = world['crossing'][0]
    N = nat.GIVE_WAY_MAX_NPCS + 1
    size, state = torch.ones((1, N, 2), device=DEV), torch.zeros((1, N, 4), device=DEV)
    with pytest.raises(nat.TdsError) as e:
        LaneFollowingNPCController(m, size, state, seed=1, give_way=True)
    assert e.value.code == nat.E_LIMIT
    ctrl = LaneFollowingNPCController(m, size, state, seed=1)                # without the option 1025 NPCs are what they were
    lanes = ctrl._lane_table_set()
    stop_at, yield_to = torch.full((1, N), 7.0, dtype=torch.float64, device=DEV), torch.full((1, N), 7, dtype=torch.int32, device=DEV)
    with pytest.raises(nat.TdsError) as e:
        _ops.lane_give_way(lanes, ctrl.scene_ids, lanes.conflict_tables(), ctrl.lane, ctrl.arc, ctrl.hops, ctrl.npc_state, ctrl.npc_size, ctrl.npc_present_mask,
                           None, 1, stop_at, yield_to)
    assert e.value.code == nat.E_LIMIT
    rc = nat.lib().tds_lane_give_way_multi(lanes.handle, None, None, None, 1, N, *([None] * 6), 0, None, None, None, 1, 60.0, 6.0, 1.0, None, None, None)
    assert rc == nat.E_LIMIT and 'NPCs' in nat.last_error()
    rc = nat.lib().tds_lane_give_way_multi(lanes.handle, None, None, None, 1, 4, *([None] * 6), 0, None, None, None, 1, 60.0, 6.0, 0.0, None, None, None)
    assert rc == nat.E_INVAL and 'creep_speed' in nat.last_error()
    with pytest.raises(nat.TdsError) as e:
        LaneFollowingNPCController(m, size[:, :4], state[:, :4], seed=1, give_way=True, creep_speed=0.0)
    assert e.value.code == nat.E_INVAL
    torch.cuda.synchronize()
    assert bool((stop_at == 7.0).all()) and bool((yield_to == 7).all()), 'a refused call wrote nothing'
