"""Traffic lights on the device (csrc/lights.hip; traffic_controls.ProgrammedTrafficLightControl, Simulator.compute_stop_lines) against the models
of their definitions (tests/lights_model.py), the reference's recorded trace on Town01 (tests/golden/g12_traffic_lights.json) and the host classes
of traffic_lights.py.

The bar: phases, sequence numbers, colours and indices equal; remaining times equal as float64, time_to_change and the stop-line features equal as
binary32 BIT PATTERNS (the programmes are float64 + - and comparisons, the stop lines binary32 + - * and one correctly rounded square root, built
with -ffp-contract=off; the models do the same operations in the same order).  No row is excepted."""
import ctypes
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import lane_follow_model as lf
import lights_model as lm
from conftest import GOLDEN
from test_gpu_lane_follow import make_sim as make_npc_sim, pose_row
from test_gpu_range_scan import make_sim
from test_lights_model import NAMES, host_controller, positions

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOWN01 = os.path.join(GOLDEN, 'maps', 'carla_Town01')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernel_tables(t):
    return dev(t['duration']), dev(t['next_phase']), dev(t['n_phases']), dev(t['colour'])


def bits(a):
    """the bit patterns of a float array (so that -0.0 and 0.0 differ and a NaN equals itself)"""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def assert_lights(got, model, what):
    """got: an object or dict with phase, remaining, state, time_to_change on the device; model: lights_model.Lights"""
    for k in ('phase', 'remaining', 'state', 'time_to_change'):
        g, w = bits(got[k] if isinstance(got, dict) else getattr(got, k)), bits(getattr(model, k))
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype)
        bad = np.argwhere(g != w)
        assert not len(bad), f'{what}: {k} differs at {bad[:6].tolist()}: kernel {g[tuple(bad[0])]}, model {w[tuple(bad[0])]}'


def town01_controller():
    from torchdrivesim_amd.traffic_lights import TrafficLightController
    return TrafficLightController.from_json(os.path.join(TOWN01, 'carla_Town01_traffic_light_controller.json'))


# ---------------------------------------------------------------------------------------------------------------- 1. the recorded trace
def test_scene_0_replays_the_reference_and_the_other_scenes_keep_their_own_clocks():
    from torchdrivesim_amd.traffic_controls import ProgrammedTrafficLightControl
    from torchdrivesim_amd.traffic_lights import current_light_state_tensor_from_controller
    g = json.load(open(os.path.join(GOLDEN, 'g12_traffic_lights.json')))
    random.seed(g['seed'])
    hosts = [town01_controller() for _ in range(3)]                     # scene 0: the reference's own start (its random.randint reset)
    control = ProgrammedTrafficLightControl(torch.zeros(3, 36, 5, device=DEV), hosts[0], g['ids'])

    def rows_of(rows):
        """the rows of a set_to of the script for scene 0, other rows (out-of-range indices and times among them) for scenes 1 and 2"""
        return [rows, [[i + 1, 0.5 * t + 0.25] for i, t in rows], [[i - 2, t + 1.0 + m] for m, (i, t) in enumerate(rows)]]

    def set_to(rows):
        per_scene = rows_of(rows)
        control.set_to(torch.tensor(per_scene, dtype=torch.float64))
        for h, r in zip(hosts[1:], per_scene[1:]):
            h.set_to(r)

    def check(want):
        per_machine, left, state = control.state_per_machine.cpu(), control.time_remaining.cpu(), control.state.cpu()
        assert left.dtype == torch.float64 and state.dtype == torch.int64
        assert per_machine[0].tolist() == want['state_per_machine'] and left[0].tolist() == want['time_remaining'] and state[0].tolist() == want['tensor']
        for b in (1, 2):
            assert per_machine[b].tolist() == hosts[b].state_per_machine and left[b].tolist() == hosts[b].time_remaining
            assert state[b].tolist() == current_light_state_tensor_from_controller(hosts[b], g['ids']).tolist()
        apart.append(left[1].tolist() != left[0].tolist() != left[2].tolist() != left[1].tolist())
    apart = []
    set_to([[p, r] for p, r in zip(positions(hosts[0]), hosts[0].time_remaining)])
    check(g['trace'][0])
    state = control.state
    for (op, arg), want in zip(g['script'], g['trace'][1:]):
        if op == 'set_to':
            set_to(arg)
        else:
            control.tick(arg)
            for h in hosts[1:]:
                h.tick(arg)
        check(want)
    assert control.state is state and len(g['trace']) == 76                                  # written in place, never replaced
    assert all(apart)                             # three clocks, at every point of the trace
    control.set_to(g['script'][0][1])             # the host's list form goes to every scene
    assert control.time_remaining[0].tolist() == control.time_remaining[1].tolist() == control.time_remaining[2].tolist() == g['trace'][1]['time_remaining']


# ---------------------------------------------------------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize('M,P,N', [(1, 1, 1), (12, 6, 36), (65, 7, 65), (3, 64, 130)])
def test_mixed_ticks_equal_the_model_at_every_shape(M, P, N):
    from torchdrivesim_amd import _ops
    B = 5
    programmes, ids = lm.random_programmes(7 * M + P, M, P, N, exact=True)
    t = lm.tables(programmes, ids)
    model = lm.Lights(t, B)
    g = np.random.default_rng(M + N)
    for b in range(B):
        model.set_to([[int(g.integers(0, P)), float(g.integers(0, 80)) / 8.0] for _ in range(M)], scenes=[b])
    tables = kernel_tables(t)
    got = dict(phase=dev(model.phase), remaining=dev(model.remaining), state=dev(model.state), time_to_change=dev(model.time_to_change))
    steps = [0.0, 0.125, 0.125, 0.5] + [float(x) for x in g.choice([0.0, 0.1, 0.125, 0.25, 3.0, 40.0, 200.0], 36)]
    for i, dt in enumerate(steps):
        mask = None if i % 4 else g.random(B) < 0.6
        before = {k: v.clone() for k, v in got.items()}
        _ops.lights_step(tables, got['phase'], got['remaining'], got['state'], got['time_to_change'], dt, mask=None if mask is None else dev(mask))
        model.tick(dt, mask=mask)
        assert_lights(got, model, f'tick {i} of {dt} s')
        if mask is not None:                      # the other scenes' rows are untouched bit for bit
            keep = dev(~mask)
            assert all(torch.equal(v[keep].view(torch.uint8), before[k][keep].view(torch.uint8)) for k, v in got.items())
    assert len(steps) == 40


def test_limits_and_arguments_are_refused_before_any_launch():
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops

    def step(M, P, N, dt, B=1):
        nat.call('tds_lights_step', torch.device(DEV), None, None, None, None, None, None, None, None, None, B, M, P, N, ctypes.byref(ctypes.c_double(dt)), 1)
    for M, P, N in ((257, 1, 1), (1, 65, 1), (1, 1, 1025)):
        with pytest.raises(nat.TdsError, match='at most') as err:
            step(M, P, N, 0.1)
        assert err.value.code == nat.E_LIMIT
    for M, P in ((257, 1), (1, 65)):
        with pytest.raises(nat.TdsError, match='at most') as err:
            nat.call('tds_lights_reset', torch.device(DEV), None, None, None, None, None, None, 1, M, P, 0)
        assert err.value.code == nat.E_LIMIT
    for dt in (-0.1, math.nan, math.inf):
        with pytest.raises(nat.TdsError, match='dt') as err:
            step(1, 1, 1, dt)
        assert err.value.code == nat.E_INVAL
    step(256, 64, 1024, 0.1, B=0)                 # an empty batch at the limits: a successful no-op
    t = lm.tables(*lm.random_programmes(1, 2, 3, 4))
    got = dict(phase=torch.zeros(1, 2, dtype=torch.int32, device=DEV), remaining=torch.ones(1, 2, dtype=torch.float64, device=DEV),
               state=torch.zeros(1, 4, dtype=torch.int64, device=DEV), time_to_change=torch.zeros(1, 4, device=DEV))
    with pytest.raises(nat.TdsError, match='dt') as err:
        _ops.lights_step(kernel_tables(t), got['phase'], got['remaining'], got['state'], got['time_to_change'], -1.0)
    assert err.value.code == nat.E_INVAL and float(got['remaining'].sum()) == 2.0


# ---------------------------------------------------------------------------------------------------------------- 3. reset
def test_reset_deals_the_models_phases_and_touches_nothing_else():
    from torchdrivesim_amd.traffic_controls import ProgrammedTrafficLightControl
    B, M, P, N, seed = 6, 12, 7, 36, 5
    programmes, ids = lm.random_programmes(77, M, P, N)
    t, host = lm.tables(programmes, ids), host_controller(programmes)
    pos = torch.zeros(B, N, 5, device=DEV)
    control = ProgrammedTrafficLightControl(pos, host, ids, seed=seed)
    model = lm.Lights(t, B)
    model.reset(seed, list(range(B)))
    assert_lights(control, model, 'the constructor ends with a reset')
    assert control.scene_ids.tolist() == list(range(B)) and len({tuple(r) for r in model.phase.tolist()}) > 1
    # a masked reset with new scene ids: the other rows stay as they are
    control.tick(0.7)
    model.tick(0.7)
    mask, new_ids = np.array([True, False, True, True, False, False]), [100, 101, 2 ** 40 + 2, 103, 104, 105]
    state = control.state
    control.reset(mask=dev(mask), scene_ids=torch.tensor(new_ids, device=DEV))
    model.reset(seed, new_ids, mask=mask)
    assert_lights(control, model, 'a masked reset')
    assert control.scene_ids.tolist() == new_ids and control.state is state
    # sub-batches reproduce the rows of the whole batch
    control.reset()
    model.reset(seed, new_ids)
    assert_lights(control, model, 'a reset of every scene')
    part = control.select_batch_elements(torch.tensor([2, 0], device=DEV), in_place=False)
    fresh = ProgrammedTrafficLightControl(pos[:2], host, ids, seed=seed, scene_ids=torch.tensor([new_ids[2], new_ids[0]], device=DEV))
    for k in ('phase', 'remaining', 'state', 'time_to_change', 'scene_ids'):
        assert torch.equal(getattr(part, k), getattr(fresh, k)) and torch.equal(getattr(part, k), getattr(control, k)[[2, 0]]), k
    # the call after a reset continues from the new phases
    control.tick(0.3)
    model.tick(0.3)
    assert_lights(control, model, 'a tick after the reset')
    other = ProgrammedTrafficLightControl(pos, host, ids, seed=seed + 1)
    assert not torch.equal(other.phase, ProgrammedTrafficLightControl(pos, host, ids, seed=seed).phase)


# ---------------------------------------------------------------------------------------------------------------- 4. through the simulator
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


@pytest.fixture(scope='module')
def package():
    from torchdrivesim_amd.map import load_map_config
    cfg = load_map_config(os.path.join(TOWN01, 'metadata.json'))
    return cfg, [s.actor_id for s in cfg.stoplines if s.agent_type == 'traffic_light']


def at_the_lights(cfg):
    """edit(states, present) of make_sim: every agent two metres past the centre of a traffic light's stop line, along the line's orientation"""
    lights = [s for s in cfg.stoplines if s.agent_type == 'traffic_light']

    def edit(states, present):
        for b in range(states.shape[0]):
            for a in range(states.shape[1]):
                s = lights[(7 * b + 3 * a) % len(lights)]
                states[b, a] = torch.tensor([s.x + 2.0 * math.cos(s.orientation), s.y + 2.0 * math.sin(s.orientation), s.orientation, 0.0], device=DEV)
    return edit


class HostFed:
    """the host path of examples/step_loop.py for B scenes with clocks of their own: B host controllers, one index tensor per step"""

    def __init__(self, control, programmed, ids):
        from torchdrivesim_amd.traffic_lights import current_light_state_tensor_from_controller
        self.control, self.ids, self.tensor = control, ids, current_light_state_tensor_from_controller
        self.hosts = [town01_controller() for _ in range(programmed.phase.shape[0])]
        for h, phase, left in zip(self.hosts, programmed.phase.tolist(), programmed.remaining.tolist()):
            h.set_to([[p, r] for p, r in zip(phase, left)])
        self.feed()

    def feed(self):
        self.control.set_state(torch.stack([self.tensor(h, self.ids) for h in self.hosts]).to(DEV))

    def tick(self, dt):
        for h in self.hosts:
            h.tick(dt)
        self.feed()


def test_a_simulator_with_programmed_lights_equals_its_host_fed_twin(town01, package):
    from torchdrivesim_amd.map import programmed_traffic_lights_from_map_config, traffic_controls_from_map_config
    cfg, ids = package
    B, A = 2, 2
    sim, twin = (make_sim(town01, [0] * B, A, seed=31, edit=at_the_lights(cfg)) for _ in range(2))
    programmed = programmed_traffic_lights_from_map_config(cfg, B, DEV, dt=0.1, seed=9)
    plain = traffic_controls_from_map_config(cfg)['traffic_light'].extend(B).to(DEV)
    assert programmed.pos.shape == plain.pos.shape == (B, len(ids), 5) and programmed.light_ids == ids and torch.equal(programmed.pos, plain.pos)
    assert not torch.equal(programmed.phase[0], programmed.phase[1])                         # two scenes, two clocks
    sim.traffic_controls, twin.traffic_controls = {'traffic_light': programmed}, {'traffic_light': plain}
    fed = HostFed(plain, programmed, ids)
    assert torch.equal(plain.state, programmed.state)
    first, state = programmed.state.clone(), programmed.state
    action = torch.zeros(B, A, 2, device=DEV)
    violations = 0
    for it in range(260):
        sim.step(action)                          # ticks the programmes on the device
        twin.step(action)
        fed.tick(0.1)                             # the twin's colours for the state both simulators are now in
        assert torch.equal(plain.state, programmed.state), it
        v = sim.compute_traffic_lights_violations()
        assert torch.equal(v, twin.compute_traffic_lights_violations()), it
        violations += int((v > 0).sum())
        if it % 26 == 7:
            assert torch.equal(sim.render_egocentric(), twin.render_egocentric()), it
    assert programmed.state is state and bool((programmed.state != first).any())            # in place, and the colours did change
    assert programmed.remaining.cpu().tolist() == [h.time_remaining for h in fed.hosts]
    print(f'{violations} red-light violations over 260 steps')
    # the batch plumbing keeps phases and times
    keys = ('phase', 'remaining', 'state', 'time_to_change', 'scene_ids')
    lights = lambda s: s.traffic_controls['traffic_light']
    copy = sim.copy()
    assert all(torch.equal(getattr(lights(copy), k), getattr(programmed, k)) and getattr(lights(copy), k).data_ptr() != getattr(programmed, k).data_ptr()
               for k in keys)
    wide = sim.extend(2, in_place=False)
    assert all(torch.equal(getattr(lights(wide), k), getattr(programmed, k)[[0, 0, 1, 1]]) for k in keys)
    one = sim.select_batch_elements([1], in_place=False)
    assert all(torch.equal(getattr(lights(one), k), getattr(programmed, k)[[1]]) for k in keys)
    moved = copy.to(DEV)
    assert all(torch.equal(getattr(lights(moved), k), getattr(programmed, k)) for k in keys)
    for s in (copy, wide, one):                   # ... and they go on from there, each with its own clocks
        s.step(torch.zeros(s.batch_size, A, 2, device=DEV))
    sim.step(action)
    assert torch.equal(lights(copy).remaining, programmed.remaining) and torch.equal(lights(wide).remaining, programmed.remaining[[0, 0, 1, 1]])
    assert torch.equal(lights(one).state, programmed.state[[1]]) and torch.equal(lights(one).remaining, programmed.remaining[[1]])


# ---------------------------------------------------------------------------------------------------------------- 5. graphs
def test_a_captured_step_and_a_captured_reset_replay_the_eager_run(town01, package):
    from torchdrivesim_amd.map import programmed_traffic_lights_from_map_config
    cfg, ids = package
    B, A = 3, 2
    live, ref = (make_sim(town01, [0] * B, A, seed=41) for _ in range(2))
    for s in (live, ref):
        s.traffic_controls = {'traffic_light': programmed_traffic_lights_from_map_config(cfg, B, DEV, dt=0.1, seed=4)}
    mine, theirs = live.traffic_controls['traffic_light'], ref.traffic_controls['traffic_light']
    action = torch.zeros(B, A, 2, device=DEV)
    state = live.get_state().clone()              # the captured step reads its pose from here, as tests/test_gpu_neighbors.py does

    def step():
        live.kinematic_model.set_state(state)
        live.step(action)
        return live.get_state()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
            theirs.tick(0.1)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        new = step()
        state_next = new.clone()
    first = theirs.state.clone()
    for i in range(60):
        ref.kinematic_model.set_state(state.clone())
        ref.step(action)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(mine, k), getattr(theirs, k)) for k in ('phase', 'remaining', 'state', 'time_to_change')), i
        assert torch.equal(new, ref.get_state()), i
        state.copy_(state_next)
    assert bool((theirs.state != first).any())
    # a reset of some scenes and a tick in one graph
    mask = torch.tensor([True, False, True], device=DEV)
    with torch.cuda.stream(s):
        mine.reset(mask=mask)
        mine.tick(0.1)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        mine.reset(mask=mask)
        mine.tick(0.1)
    for k in ('phase', 'remaining', 'state', 'time_to_change'):
        getattr(mine, k).copy_(getattr(theirs, k))
    for i in range(2):
        g2.replay()
        theirs.reset(mask=mask)
        theirs.tick(0.1)
        torch.cuda.synchronize()
        assert all(torch.equal(getattr(mine, k), getattr(theirs, k)) for k in ('phase', 'remaining', 'state', 'time_to_change')), i
    model = lm.Lights(lm.tables(json.loads(town01_controller().to_json()), ids), B)
    model.reset(4, [0, 1, 2])
    model.tick(0.1)
    assert mine.phase[[0, 2]].tolist() == model.phase[[0, 2]].tolist() and mine.remaining[[0, 2]].tolist() == model.remaining[[0, 2]].tolist()


# ---------------------------------------------------------------------------------------------------------------- 6. stop lines
def run(c, k, max_distance, **kw):
    from torchdrivesim_amd import _ops
    t = {key: None if v is None else dev(v) for key, v in c.items()}
    out = _ops.stop_lines(t['agent_xy'], t['agent_sc'], t['agent_present'], t['lines'], t['line_sc'], t['mask'], t['state'], t['time_to_change'], k,
                          max_distance, **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == out[2].dtype == torch.int32 and not out[0].requires_grad
    return tuple(o.cpu().numpy() for o in out)


def assert_slots(got, want, what):
    for name, g, w in zip(('features', 'index', 'state'), got, want):
        g, w = bits(g), bits(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        bad = np.argwhere(g != w)
        assert not len(bad), f'{what}: {name} differs at {bad[:8].tolist()}: kernel {got[0][tuple(bad[0][:3])]!r}, model {want[0][tuple(bad[0][:3])]!r}'


@pytest.mark.parametrize('ahead_only,min_cos', list(lm.DEFINITION_INDEX))
def test_the_definition_cases_through_the_entry_point(ahead_only, min_cos):
    from torchdrivesim_amd import _native as nat
    c = lm.definition_cases()
    kw = dict(ahead_only=ahead_only, min_cos=min_cos)
    got = run(c, 4, lm.DEFINITION_MAX_DISTANCE, **kw)
    assert got[1].tolist() == lm.DEFINITION_INDEX[(ahead_only, min_cos)]
    assert_slots(got, lm.stop_lines(**c, k=4, max_distance=lm.DEFINITION_MAX_DISTANCE, **kw), 'definition cases')
    # every output is written in full: the same call into tensors that held something else
    t = {k: dev(v) for k, v in c.items()}
    features = torch.full((2, 3, 4, 8), float('nan'), device=DEV)
    index = torch.full((2, 3, 4), 99, dtype=torch.int32, device=DEV)
    state = torch.full((2, 3, 4), 99, dtype=torch.int32, device=DEV)
    nat.call('tds_stop_lines_f32', torch.device(DEV), t['agent_xy'], t['agent_sc'], t['agent_present'].view(torch.uint8), t['lines'], t['line_sc'],
             t['mask'].view(torch.uint8), t['state'], t['time_to_change'], features, index, state, 2, 3, 6, 4, lm.DEFINITION_MAX_DISTANCE, int(ahead_only),
             -math.inf if min_cos is None else min_cos)
    assert_slots((features.cpu().numpy(), index.cpu().numpy(), state.cpu().numpy()), got, 'into used tensors')
    without = run({**c, 'time_to_change': None}, 4, lm.DEFINITION_MAX_DISTANCE, **kw)
    assert_slots(without, lm.stop_lines(**{**c, 'time_to_change': None}, k=4, max_distance=lm.DEFINITION_MAX_DISTANCE, **kw), 'no time_to_change')


@pytest.mark.parametrize('N', [6, 64, 65, 130])
def test_wave_and_stride_boundaries(N):
    """one lane per line up to 64, the strided rounds above; K = 1, 4 and 32 (more slots than lines at N = 6); random float32 poses in a 120 m square
    with duplicated positions; a radius and none"""
    B, A = 2, 5
    s = lm.random_scenes(200 + N, B, A, N)
    filled = 0
    for K in (1, 4, 32):
        for max_distance in (30.0, float('inf')):
            want = lm.stop_lines(**s, k=K, max_distance=max_distance, ahead_only=False)
            assert_slots(run(s, K, max_distance, ahead_only=False), want, f'N={N} K={K} max_distance={max_distance}')
            filled += int((want[1] >= 0).sum())
    assert filled > 0


@pytest.mark.parametrize('A', [16, 17, 33])
def test_slices_of_observers_and_the_later_turns_of_a_wave(A):
    """a workgroup takes 16 observers, four per wave: one full slice, a second slice with one observer, a third; B = 2, K = 4, 40 lines (by rank)
    and 70 (in rounds), a fifth of the observers and of the lines absent"""
    for N in (40, 70):
        s = lm.random_scenes(5000 + 100 * A + N, 2, A, N, absent=0.2)
        want = lm.stop_lines(**s, k=4, max_distance=60.0, ahead_only=False)
        assert not s['agent_present'].all() and (want[1][:, 16 * ((A - 1) // 16):] >= 0).any()         # absent observers; the last slice sees a line
        assert_slots(run(s, 4, 60.0, ahead_only=False), want, f'A={A} N={N}')


def test_the_line_limit_and_the_arguments():
    from torchdrivesim_amd import _native as nat
    s = lm.random_scenes(9, 1, 2, 1024, duplicates=0.02)
    s['agent_present'][:] = True
    want = lm.stop_lines(**s, k=32, max_distance=60.0, ahead_only=False)
    assert (want[1] >= 0).all()
    assert_slots(run(s, 32, 60.0, ahead_only=False), want, 'N=1024')
    with pytest.raises(nat.TdsError, match='LDS') as err:
        run(lm.random_scenes(8, 1, 2, 1025), 32, 50.0)
    assert err.value.code == nat.E_LIMIT
    small = lm.random_scenes(8, 1, 2, 5)
    for k, max_distance, min_cos in ((0, 10.0, None), (33, 10.0, None), (4, -1.0, None), (4, math.nan, None), (4, 10.0, math.nan)):
        with pytest.raises(ValueError):
            run(small, k, max_distance, min_cos=min_cos)
    t = {k: dev(v) for k, v in small.items()}
    out = torch.zeros(1, 2, 4, 8, device=DEV), torch.zeros(1, 2, 4, dtype=torch.int32, device=DEV), torch.zeros(1, 2, 4, dtype=torch.int32, device=DEV)
    for k, max_distance, min_cos in ((0, 10.0, 0.0), (33, 10.0, 0.0), (4, -1.0, 0.0), (4, math.nan, 0.0), (4, 10.0, math.nan)):
        with pytest.raises(nat.TdsError) as err:
            nat.call('tds_stop_lines_f32', torch.device(DEV), t['agent_xy'], t['agent_sc'], t['agent_present'].view(torch.uint8), t['lines'], t['line_sc'],
                     t['mask'].view(torch.uint8), t['state'], None, *out, 1, 2, 5, k, max_distance, 1, min_cos)
        assert err.value.code == nat.E_INVAL


def test_the_two_filters_remove_what_the_model_removes():
    s = lm.random_scenes(55, 3, 6, 40, side=60.0)
    plain = run(s, 8, 40.0, ahead_only=False)
    for kw in (dict(ahead_only=True), dict(ahead_only=False, min_cos=0.3), dict(ahead_only=True, min_cos=-0.2)):
        got = run(s, 8, 40.0, **kw)
        assert_slots(got, lm.stop_lines(**s, k=8, max_distance=40.0, **kw), str(kw))
        assert (got[1] != plain[1]).any()
        b, a, k = np.nonzero(got[1] >= 0)
        if kw['ahead_only']:
            assert (got[0][b, a, k, 0] >= 0).all()
        if 'min_cos' in kw:
            assert (got[0][b, a, k, 3] >= np.float32(kw['min_cos'])).all()


def stop_line_inputs(sim, control):
    """exactly what compute_stop_lines hands to the kernel, as the model's arguments"""
    from torchdrivesim_amd import _ops
    st, A = sim.get_state(), sim.agent_count
    ttc = getattr(control, 'time_to_change', None)
    return dict(agent_xy=st[..., :2].cpu().numpy(), agent_sc=sim._heading_sc()[:, :A].cpu().numpy(), agent_present=sim.get_present_mask().cpu().numpy(),
                lines=control.pos.cpu().numpy(), line_sc=_ops.heading_sc(control.pos[..., 4].contiguous()).cpu().numpy(),
                mask=control.mask.cpu().numpy(), state=control.state.cpu().numpy(), time_to_change=None if ttc is None else ttc.cpu().numpy())


def as_numpy(sl):
    return sl.features.cpu().numpy(), sl.index.cpu().numpy(), sl.state.cpu().numpy()


def test_stop_lines_through_the_simulator(town01, package):
    from torchdrivesim_amd.map import programmed_traffic_lights_from_map_config, traffic_controls_from_map_config
    from torchdrivesim_amd.simulator import StopLines
    from torchdrivesim_amd.traffic_controls import StopSignControl
    cfg, ids = package
    B, A = 2, 4
    sim = make_sim(town01, [0] * B, A, seed=31, edit=at_the_lights(cfg))
    with pytest.raises(ValueError, match='traffic controls'):
        sim.compute_stop_lines()
    control = programmed_traffic_lights_from_map_config(cfg, B, DEV, seed=2)
    signs = StopSignControl(control.pos[:, :5].clone())
    sim.traffic_controls = {'traffic_light': control, 'stop_sign': signs}
    control.tick(3.3)
    sl = sim.compute_stop_lines(k=4, max_distance=60.0, ahead_only=False)
    assert isinstance(sl, StopLines) and sl.features.shape == (B, A, 4, 8) and sl.index.shape == sl.state.shape == (B, A, 4)
    assert StopLines.FEATURES[6:] == ('time_to_change', 'distance')
    assert_slots(as_numpy(sl), lm.stop_lines(**stop_line_inputs(sim, control), k=4, max_distance=60.0, ahead_only=False), 'compute_stop_lines')
    assert bool(sl.mask[:, :, 0].all()) and torch.equal(sl.mask, sl.index >= 0)          # every agent stands at a light
    assert torch.equal(sl.take(control.time_to_change), sl.features[..., 6]) and bool((sl.features[..., 6][sl.mask] > 0).all())
    assert torch.equal(sl.take(control.state, fill=-1).to(torch.int32), sl.state)
    assert_slots(as_numpy(sim.compute_stop_lines()), lm.stop_lines(**stop_line_inputs(sim, control), k=4, max_distance=60.0), 'the defaults')
    # a control without a programme: the state it holds, no time; other kinds of control
    plain = traffic_controls_from_map_config(cfg)['traffic_light'].extend(B).to(DEV)
    plain.set_state(torch.randint(0, 3, plain.state.shape, device=DEV))
    sim.traffic_controls['traffic_light'] = plain
    got = sim.compute_stop_lines(k=3, max_distance=80.0, min_cos=0.0)
    assert_slots(as_numpy(got), lm.stop_lines(**stop_line_inputs(sim, plain), k=3, max_distance=80.0, min_cos=0.0), 'a plain control')
    assert bool((got.features[..., 6] == 0).all()) and bool(got.mask.any())
    got = sim.compute_stop_lines(k=2, kind='stop_sign', ahead_only=False, max_distance=float('inf'))
    assert_slots(as_numpy(got), lm.stop_lines(**stop_line_inputs(sim, signs), k=2, max_distance=float('inf'), ahead_only=False), 'stop signs')
    assert bool(got.mask.all()) and bool((got.state == 0).all())
    # captured with a step, replayed
    sim.traffic_controls['traffic_light'] = control
    action = torch.zeros(B, A, 2, device=DEV)

    def step():
        sim.step(action)
        return sim.compute_stop_lines(k=4, max_distance=60.0, ahead_only=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert_slots(as_numpy(captured), lm.stop_lines(**stop_line_inputs(sim, control), k=4, max_distance=60.0, ahead_only=False), f'replay {i}')
        eager = sim.compute_stop_lines(k=4, max_distance=60.0, ahead_only=False)
        assert_slots(as_numpy(captured), as_numpy(eager), f'replay {i} against eager')


# ---------------------------------------------------------------------------------------------------------------- 7. NPCs
def test_an_npc_waits_for_the_programme_to_turn_its_light_green(package):
    """Town01's own stop lines and programmes, on `revert_map` of the town (tests/test_gpu_lane_follow.py): an NPC 20 m before a light that the
    programme keeps red for at least 15 s stands in front of it, drives on once the programme turns the light green, and does both at the very steps
    of a twin whose plain control is fed from a host controller."""
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.map import programmed_traffic_lights_from_map_config, traffic_controls_from_map_config
    cfg, ids = package
    reverted = lanelet2.revert_map(lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'carla_Town01.osm.gz'), origin=(0.0, 0.0)))
    m = lf.Lanes(reverted)
    towns = ([reverted], [m])
    programmed = programmed_traffic_lights_from_map_config(cfg, 1, DEV, dt=0.1, seed=1)
    plain = traffic_controls_from_map_config(cfg)['traffic_light'].to(DEV)
    pos = plain.pos[0].cpu().numpy()
    red, green = NAMES.index('red'), NAMES.index('green')
    # a start of the programmes (every machine at the beginning of phase p) and a light on a centre line 22 m into a lanelet that is red for the
    # first 15 .. 40 s and green right after, by the model
    t = lm.tables(json.loads(town01_controller().to_json()), ids)
    found = None
    for p in range(6):
        model = lm.Lights(t, 1)
        model.set_to([[p, 1000.0]] * 12)
        colours = [model.state[0].copy()]
        for _ in range(400):
            model.tick(0.1)
            colours.append(model.state[0].copy())
        colours = np.stack(colours)
        for k, (x, y) in enumerate(pos[:, :2]):
            turns = np.nonzero(colours[:, k] != red)[0]
            if not len(turns) or not 150 <= turns[0] <= 400 or colours[turns[0], k] != green:
                continue
            for l in range(len(m)):
                if not m.eligible(l) or m.length(l) < 25.0:
                    continue
                kk, u, tx, ty = lf.foot(m.cl[l], float(x), float(y))
                fx, fy = m.cl[l][kk][0] + u * (m.cl[l][kk + 1][0] - m.cl[l][kk][0]), m.cl[l][kk][1] + u * (m.cl[l][kk + 1][1] - m.cl[l][kk][1])
                arc = m.cum[l][kk] + u * (m.cum[l][kk + 1] - m.cum[l][kk])
                if math.hypot(fx - x, fy - y) < 0.5 and arc > 22.0:
                    found = (p, k, l, arc, int(turns[0]))
                    break
            if found:
                break
        if found:
            break
    assert found, 'no traffic light on a centre line 22 m into a lanelet is red for 15 s and then green'
    p, k, l, stop_arc, t_green = found

    def edit(states, present):
        states[0, 1] = torch.tensor(pose_row(m, l, stop_arc - 20.0, 8.0), device=DEV)
        states[0, 0] = torch.tensor([5000.0, 5000.0, 0.0, 0.0], device=DEV)
    sim, twin = (make_npc_sim(towns, [0], 1, 1, seed=503, edit=edit, obey_traffic_lights=True) for _ in range(2))
    programmed.set_to([[p, 1000.0]] * 12)
    sim.traffic_controls, twin.traffic_controls = {'traffic_light': programmed}, {'traffic_light': plain}
    fed = HostFed(plain, programmed, ids)
    assert sim.npc_controller.lane[0, 0].item() == l and programmed.state[0, k].item() == red
    zero = torch.zeros((1, 1, 2), device=DEV)
    speeds = []
    for it in range(t_green + 60):
        sim.step(zero)
        twin.step(zero)
        fed.tick(0.1)
        assert torch.equal(plain.state, programmed.state) and torch.equal(sim.npc_controller.npc_state, twin.npc_controller.npc_state), it
        assert programmed.state[0, k].item() == (red if it + 1 < t_green else green), it
        speeds.append(sim.npc_controller.npc_state[0, 0, 3].item())
    ctrl = sim.npc_controller
    # the NPC of step `it` sees the colours of before that step's tick: red up to and including step t_green - 1, green from step t_green
    assert max(speeds[t_green - 10:t_green]) == 0.0 and speeds[t_green] > 0.0                 # it stands while the light is red ...
    assert speeds[-1] > 3.0 and (ctrl.hops[0, 0].item() > 0 or ctrl.arc[0, 0].item() > stop_arc + 2.0)          # ... and has moved on after green
    assert torch.equal(ctrl.arc, twin.npc_controller.arc) and torch.equal(ctrl.hops, twin.npc_controller.hops)
