"""The numpy models of the device traffic lights (tests/lights_model.py: the programmes over their tables, the stop-line selection) against the
reference's recorded trace on Town01 (tests/golden/g12_traffic_lights.json), against the host classes of traffic_lights.py on random programmes
and against hand-written answers; plus the table builder and the ValueErrors of ProgrammedTrafficLightControl.  CPU only."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import lights_model as lm
import spawn_model as sm
from torchdrivesim_amd.traffic_controls import ProgrammedTrafficLightControl, light_programme_tables
from torchdrivesim_amd.traffic_lights import (TrafficLightController, TrafficLightStateMachine, _phase_from_json,
                                              current_light_state_tensor_from_controller)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = list(lm.ALLOWED)


def host_controller(programmes):
    return TrafficLightController([TrafficLightStateMachine([_phase_from_json(it) for it in prog]) for prog in programmes])


def positions(ctl):
    """the LIST POSITION of every machine's current phase"""
    return [next(i for i, s in enumerate(fsm.states) if s is fsm.current_state) for fsm in ctl.traffic_fsms]


def same_tables(package, model):
    assert sorted(package) == sorted(model)
    for k, v in model.items():
        got = package[k].numpy()
        assert got.dtype == v.dtype and got.shape == v.shape and (got == v).all(), k


def test_the_tables_and_the_tick_replay_the_reference_on_town01():
    g = json.load(open(os.path.join(GOLD, 'g12_traffic_lights.json')))
    t = lm.tables(g['to_json'], g['ids'])
    random.seed(g['seed'])
    ctl = TrafficLightController.from_json(os.path.join(GOLD, 'maps', 'carla_Town01', 'carla_Town01_traffic_light_controller.json'))
    same_tables(light_programme_tables(ctl, g['ids'], NAMES), t)
    assert t['duration'].shape == (12, 6) and t['colour'].shape == (12, 6, 36)
    lights = lm.Lights(t, 1)
    lights.phase[0], lights.remaining[0] = positions(ctl), ctl.time_remaining
    lights.refresh()

    def check(want):
        assert lights.state_per_machine[0].tolist() == want['state_per_machine']
        assert lights.remaining[0].tolist() == want['time_remaining']            # float64 ==
        assert lights.state[0].tolist() == want['tensor']
    check(g['trace'][0])
    for (op, arg), want in zip(g['script'], g['trace'][1:]):
        getattr(lights, op)(arg)
        check(want)
    assert len(g['trace']) == 76 and len(g['script']) == 75
    ops = [op for op, _ in g['script']]
    assert ops.count('set_to') >= 2 and ['tick', 0.0] in g['script']


@pytest.mark.parametrize('M,P,N,exact', [(1, 1, 1, True), (1, 7, 5, False), (12, 1, 30, False), (12, 7, 36, True), (12, 7, 36, False)])
def test_the_model_equals_the_host_controller_on_random_programmes(M, P, N, exact):
    programmes, ids = lm.random_programmes(1000 * M + 10 * P + exact, M, P, N, exact=exact)
    ctl = host_controller(programmes)
    t = lm.tables(programmes, ids)
    same_tables(light_programme_tables(ctl, ids, NAMES), t)
    lights = lm.Lights(t, 1)
    g = np.random.default_rng(M + P)
    start = [[int(g.integers(-1, P + 2)), float(g.integers(0, 100)) / 8.0] for _ in range(M)]
    ctl.set_to(start)
    lights.set_to(start)
    cycle = max(sum(ph['duration'] for ph in prog) for prog in programmes)       # the longest machine's own loop, at most 7 x 9 s
    steps = [0.125] * 60 + [0.0, 1.0, 2.5, 3.0 * cycle, 0.125, 6.0 * cycle + 0.375] + ([float(x) for x in g.uniform(0, 12, 40)] if not exact else [0.25] * 40)
    fresh = 0
    for dt in steps:
        ctl.tick(dt)
        lights.tick(dt)
        assert lights.remaining[0].tolist() == ctl.time_remaining, dt
        assert lights.state_per_machine[0].tolist() == ctl.state_per_machine and lights.phase[0].tolist() == positions(ctl)
        assert lights.state[0].tolist() == current_light_state_tensor_from_controller(ctl, ids).tolist()
        last = {a: m for m, fsm in enumerate(ctl.traffic_fsms) for a in fsm.get_current_actor_states()}          # the later machine wins
        assert lights.time_to_change[0].tolist() == [float(np.float32(ctl.time_remaining[last[str(i)]])) for i in ids]
        fresh += sum(r == fsm.duration for r, fsm in zip(ctl.time_remaining, ctl.traffic_fsms))
    if exact:
        assert fresh > 0                          # phases that ended exactly on a tick: the `left == 0` branch
    if M > 1:
        shared = [i for i in ids if sum(any(str(i) in ph['actor_states'] for ph in prog) for prog in programmes) > 1]
        assert shared                             # ids that several machines name


def _phase(colour='red', duration=2.0, nxt=0, actor='7', seq=0):
    return dict(actor_states={actor: colour}, state=str(seq), duration=duration, next_state=str(nxt))


def test_what_the_constructor_refuses():
    pos = torch.zeros(2, 1, 5)
    good = [[_phase('red', 2.0, 1), _phase('green', 3.0, 0, seq=1)]]
    light_programme_tables(host_controller(good), [7], NAMES, 0.1)
    for bad, what in (([[_phase(duration=0.0)]], 'duration'), ([[_phase(duration=math.inf)]], 'duration'), ([[_phase(duration=math.nan)]], 'duration'),
                      ([[_phase(duration=-1.0)]], 'duration'), ([[_phase(nxt=1)]], 'next_state'), ([[_phase(nxt=-1)]], 'next_state'),
                      ([[_phase(colour='none')]], 'none'),
                      ([[_phase('red', 2.0, 1), _phase('green', 3.0, 0, actor='8')]], 'every one of its phases')):
        with pytest.raises(ValueError, match=what):
            ProgrammedTrafficLightControl(pos, host_controller(bad), [7])
    for dt in (-0.1, math.nan, math.inf, 1024 * 2.0 + 1.0):
        with pytest.raises(ValueError, match='dt must be'):
            ProgrammedTrafficLightControl(pos, host_controller(good), [7], dt=dt)
    light_programme_tables(host_controller(good), [7], NAMES, 1024 * 2.0)           # the bound itself is allowed
    with pytest.raises(ValueError, match='light ids'):
        ProgrammedTrafficLightControl(pos, host_controller(good), [7, 8])
    # a light named in every phase by NO single machine, although some machine names it at any time
    split = [[_phase('red', 2.0, 1), _phase('green', 3.0, 0, actor='8')], [_phase('red', 2.0, 1, actor='8'), _phase('green', 3.0, 0)]]
    with pytest.raises(ValueError, match='every one of its phases'):
        ProgrammedTrafficLightControl(pos, host_controller(split), [7])
    # everything in order, but the tensors are on the host: there is no CPU fallback
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ProgrammedTrafficLightControl(pos, host_controller(good), [7])


def test_the_reset_pick_is_the_spawn_generator_scaled_to_the_machine():
    seen = set()
    for seed, scene, m, n in ((0, 0, 0, 6), (0, 1, 0, 6), (0, 0, 1, 6), (1, 0, 0, 6), (2 ** 63 + 5, 2 ** 40 + 3, 11, 64), (12, 7, 255, 1), (3, 2 ** 32, 4, 7)):
        key = ((seed & 0xFFFFFFFF) ^ 0x4C494748, ((seed >> 32) & 0xFFFFFFFF) ^ 0x54535452)
        word = sm.philox4x32_10((scene & 0xFFFFFFFF, scene >> 32, m, 0), key)[0]
        got = lm.reset_phase(seed, scene, m, n)
        assert got == (int(word) * n) >> 32 and 0 <= got < n
        seen.add(int(word))
    assert len(seen) == 7                         # seed, scene id (both halves) and machine all reach the generator
    assert 0x4C494748 == int.from_bytes(b'LIGH', 'big') and 0x54535452 == int.from_bytes(b'TSTR', 'big')
    picks = [lm.reset_phase(5, b, 0, 6) for b in range(600)]
    assert sorted(set(picks)) == list(range(6)) and max(np.bincount(picks)) < 150


@pytest.mark.parametrize('ahead_only,min_cos', list(lm.DEFINITION_INDEX))
def test_the_stop_line_definition_cases(ahead_only, min_cos):
    c = lm.definition_cases()
    features, index, state = lm.stop_lines(**c, k=4, max_distance=lm.DEFINITION_MAX_DISTANCE, ahead_only=ahead_only, min_cos=min_cos)
    assert index.tolist() == lm.DEFINITION_INDEX[(ahead_only, min_cos)]
    empty = index < 0
    assert (state[empty] == -1).all() and (features[empty] == 0).all()
    assert (state[~empty] == np.take_along_axis(c['state'][:, None, :].repeat(3, 1), index.clip(0).astype(np.int64), 2)[~empty]).all()
    b, a, k = np.nonzero(~empty)
    n = index[b, a, k]
    assert (features[b, a, k, 4] == c['lines'][b, n, 2]).all() and (features[b, a, k, 5] == c['lines'][b, n, 3]).all()
    assert (features[b, a, k, 6] == c['time_to_change'][b, n]).all()
    if (ahead_only, min_cos) == (True, None):
        # observer 0 of scene 0: the tie in the order of the indices, then the line at exactly r2; line 1 is turned by pi
        assert features[0, 0, :3, 7].tolist() == [5.0, 5.0, 10.0] and features[0, 0, :3, 0].tolist() == [3.0, 3.0, 6.0]
        assert features[0, 0, :3, 1].tolist() == [4.0, -4.0, 8.0] and features[0, 0, :3, 3].tolist() == [1.0, -1.0, 1.0]
        assert features[0, 1, 0, :2].tolist() == [3.0, 0.0]                       # observer 1 looks the other way: line 4 is ahead of it
        assert features[1, 0, 0, 7] == 0.0 and features[1, 2, 0, 0] == 1.0        # on the line; one metre before it
    without = lm.stop_lines(**{**c, 'time_to_change': None}, k=4, max_distance=lm.DEFINITION_MAX_DISTANCE, ahead_only=ahead_only, min_cos=min_cos)
    assert (without[0][..., 6] == 0).all() and (without[1] == index).all()


def test_the_stop_line_model_is_sorted_and_complete_on_random_scenes():
    s = lm.random_scenes(3, 2, 4, 70)
    features, index, state = lm.stop_lines(**s, k=32, max_distance=40.0, ahead_only=False)
    assert (index >= 0).any()
    d = features[..., 7]
    for b in range(2):
        for a in range(4):
            n = int((index[b, a] >= 0).sum())
            assert (np.diff(d[b, a, :n]) >= 0).all() and (index[b, a, n:] == -1).all()
            d64 = np.hypot(*(s['lines'][b, :, :2].astype(np.float64) - s['agent_xy'][b, a].astype(np.float64)).T)
            inside = s['mask'][b] & (d64 < 39.99) & s['agent_present'][b, a]
            assert set(np.nonzero(inside)[0]) <= set(index[b, a, :n].tolist()) or n == 32
