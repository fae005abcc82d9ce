"""
The clock arithmetic the light kernel runs per machine (torchdrivesim_amd/csrc/tds_lights.h) compiled for the HOST by tests/lights_host.cpp: it
replays the reference's recorded script on Town01 (tests/golden/g12_traffic_lights.json) and random programmes, and must reproduce the trace and
the numpy model (tests/lights_model.py) in every bit of every remaining time.  The program is also built with the address and
undefined-behaviour sanitizers and run as it is.  CPU only.
"""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import lights_model as lm
from test_lights_model import GOLD, host_controller, positions
from torchdrivesim_amd.traffic_lights import TrafficLightController

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'lights_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
PICKS = [(0, 0, 0, 6), (0, 1, 0, 6), (12, 2 ** 40 + 3, 11, 64), (2 ** 63 + 5, 7, 255, 1), (3, 2 ** 32, 4, 7)]


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def run(program, script):
    r = subprocess.run([program, script], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def table_lines(t):
    M, P = t['duration'].shape
    out = [f'{M} {P}']
    for m in range(M):
        out.append(' '.join([str(int(t['n_phases'][m]))] + [float(d).hex() for d in t['duration'][m]] + [str(int(n)) for n in t['next_phase'][m]]))
    return out


def command(op, arg):
    if op == 'tick':
        return f'tick {float(arg).hex()}'
    return f'set {len(arg)} ' + ' '.join(f'{int(i)} {float(t).hex()}' for i, t in arg)


def clocks(output):
    """[(phases, remaining times)] of the program's clock lines"""
    rows = [ln.split()[1:] for ln in output.splitlines() if ln.startswith('clock ')]
    return [([int(p) for p in r[0::2]], [float.fromhex(x) for x in r[1::2]]) for r in rows]


@pytest.fixture(scope='module')
def cases():
    """the input of the program (one file per table) with what each clock line must say -> [(name, text, [(sequence numbers, remaining)])]"""
    g = json.load(open(os.path.join(GOLD, 'g12_traffic_lights.json')))
    t = lm.tables(g['to_json'], g['ids'])
    random.seed(g['seed'])
    ctl = TrafficLightController.from_json(os.path.join(GOLD, 'maps', 'carla_Town01', 'carla_Town01_traffic_light_controller.json'))
    text = table_lines(t) + ['start ' + ' '.join(f'{p} {float(r).hex()}' for p, r in zip(positions(ctl), ctl.time_remaining))]
    text += [command(op, arg) for op, arg in g['script']] + ['pick %d %d %d %d' % p for p in PICKS]
    out = [('g12', '\n'.join(text) + '\n', t, [(w['state_per_machine'], w['time_remaining']) for w in g['trace']])]
    # random programmes against the host classes themselves: binary-exact durations (phases end exactly on a tick), ticks of several cycles,
    # and one tick beyond TDS_LIGHTS_MAX_SKIPS phases, where the definition (the model) and not the uncapped host loop is the yardstick
    for exact in (True, False):
        programmes, ids = lm.random_programmes(40 + exact, 12, 7, 36, exact=exact)
        t = lm.tables(programmes, ids)
        ctl, model = host_controller(programmes), lm.Lights(t, 1)
        start = [[p, 1000.0] for p in range(12)]
        ctl.set_to(start)
        model.set_to(start)
        script = [('set', start)] + [('tick', dt) for dt in [0.125] * 50 + [0.0, 3.3, 190.0, 0.125, 377.875] + [0.25] * 20]
        want = []
        for op, arg in script:
            getattr(ctl, 'set_to' if op == 'set' else 'tick')(arg)
            want.append((ctl.state_per_machine, list(ctl.time_remaining)))
        script.append(('tick', 1.0e6))
        for op, arg in script[1:]:
            model.tick(arg)
        want.append((model.state_per_machine[0].tolist(), model.remaining[0].tolist()))
        out.append((f'random{int(exact)}', '\n'.join(table_lines(t) + [command(op, arg) for op, arg in script]) + '\n', t, want))
    return out


def check(program, cases, tmp):
    outputs = []
    for name, text, t, want in cases:
        path = os.path.join(tmp, name + '.txt')
        with open(path, 'w') as f:
            f.write(text)
        output = run(program, path)
        got = clocks(output)
        assert len(got) == len(want), name
        for i, ((phases, remaining), (seq, left)) in enumerate(zip(got, want)):
            assert [int(t['sequence_number'][m, p]) for m, p in enumerate(phases)] == list(seq), (name, i)
            assert remaining == list(left), (name, i)                       # float64 ==: every bit but the sign of a zero, which no time has
        if name == 'g12':
            assert len(got) == 76
            assert [int(ln.split()[1]) for ln in output.splitlines() if ln.startswith('pick ')] == [lm.reset_phase(*p) for p in PICKS]
        outputs.append(output)
    return outputs


def test_the_header_replays_the_trace_and_equals_the_host_classes(cases, tmp_path):
    check(build('lights_host'), cases, str(tmp_path))


def test_clean_under_the_sanitizers(cases, tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries are loaded
    program = build('lights_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    check(program, cases, str(tmp_path))
