"""
The arithmetic of giving way at junctions (torchdrivesim_amd/csrc/tds_conflicts.h) compiled for the HOST by tests/give_way_host.cpp: the conflict
tables of Town01, Town02 and the synthetic crossing, and the yield decisions of scenes of NPCs on them, must equal the numpy model
(tests/give_way_model.py) in every bit.  The program is also built with the address and undefined-behaviour sanitizers and run as it is.  CPU only.
"""
import os
import subprocess

import numpy as np
import pytest

import give_way_cases as gc
import give_way_model as gw
import lane_follow_model as lf
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'give_way_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
F32 = np.float32
SEED, HORIZON, B_MAX, CREEP = 5, 60.0, 6.0, 1.0


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def path_of(model, lane, arc, hops, scene_id, npc):
    """the lanelets of an NPC's path and where each starts: the walk of give_way_model.summary without its junction test"""
    l, start, out = lane, -arc, []
    for k in range(lf.MAX_HOPS + 1):
        out.append((l, start))
        nxt_start = start + model.length(l)
        if nxt_start >= HORIZON or k == lf.MAX_HOPS:
            break
        nxt = model.successor(l, SEED, scene_id, npc, hops + k)
        if nxt < 0:
            break
        l, start = nxt, nxt_start
    return out


def scene_on(model, tables, rng, n):
    """n NPCs on random drivable lanelets (the conflicted ones and their predecessors twice as likely), some absent, some fast, some standing; red and
    green stop lines before some of them, one on no lanelet"""
    ok = [l for l in range(len(model)) if model.eligible(l)]
    hot = [l for l in ok if tables[2][l] >= 0 or any(tables[2][s] >= 0 for s in model.succ[l])]
    lane = np.array([rng.choice(hot if hot and rng.random() < 0.66 else ok) for _ in range(n)], np.int32)
    arc = np.array([rng.uniform(0.0, model.length(int(l))) for l in lane])
    hops = rng.integers(0, 5, n).astype(np.int32)
    speed = rng.choice(np.array([0.0, 0.5, 3.0, 6.0, 6.0, 9.0, 14.0], F32), n)
    size = np.stack([rng.choice(np.array([4.5, 4.5, 5.25, 12.0], F32), n), np.full(n, 2.0, F32)], 1)
    present = rng.random(n) < 0.9
    lines = [(int(lane[k]), float(arc[k]) + 3.0, bool(rng.random() < 0.7)) for k in range(0, n, 4)] + [(-1, 3.0, True)]       # 3 m ahead of every fourth NPC
    return lane, arc, hops, speed, size, present, lines


@pytest.fixture(scope='module')
def cases():
    """[(name, the program's input, the model's tables, stop_at, yield_to)]"""
    from torchdrivesim_amd import lanelet2
    maps = {f'Town0{k}': lanelet2.load_lanelet_map(os.path.join(GOLDEN, f'carla_Town0{k}.osm.gz'), origin=(0.0, 0.0)) for k in (1, 2)}
    maps['crossing'] = gc.crossing_map()
    out = []
    for i, (name, m) in enumerate(maps.items()):
        model = lf.Lanes(m)
        clearance, step = (2.0, 0.5) if name != 'Town02' else (1.5, 0.25)
        tables = gw.conflict_tables(model, clearance, step)
        text = [f'map {len(model)}']
        for l in range(len(model)):
            c, cum = model.cl[l], model.cum[l]
            text.append(' '.join([str(len(c))] + [float(v).hex() for v in np.asarray(c).reshape(-1)] + [float(v).hex() for v in cum] +
                                 [str(len(model.succ[l]))] + [str(s) for s in model.succ[l]]))
        text.append(f'table {clearance.hex()} {step.hex()}')
        rng = np.random.default_rng(100 + i)
        n = 96 if name != 'crossing' else 24
        lane, arc, hops, speed, size, present, lines = scene_on(model, tables, rng, n)
        stop_at, yield_to, s = gw.give_way(model, tables, lane, arc, hops, speed, size, present, SEED, i, lines, HORIZON, B_MAX, CREEP)
        text.append(f'scene {n} {len(lines)} {HORIZON.hex()} {B_MAX.hex()} {CREEP.hex()}')
        text += [f'{l} {a.hex()} {int(r)}' for l, a, r in lines]
        for k in range(n):
            path = path_of(model, int(lane[k]), float(arc[k]), int(hops[k]), i, k)
            text.append(' '.join([str(int(present[k])), float(size[k][0]).hex(), float(speed[k]).hex(), str(len(path))] + [f'{l} {st.hex()}' for l, st in path]))
        assert (yield_to >= 0).sum() >= 3 and any(x is not None and x['held'] for x in s) and any(x is not None and x['committed'] for x in s), name
        out.append((name, '\n'.join(text) + '\n', tables, stop_at, yield_to))
    return out


def check(program, cases, tmp):
    for name, text, (exit_, zone_in, zone_out), stop_at, yield_to in cases:
        path = os.path.join(tmp, name + '.txt')
        with open(path, 'w') as f:
            f.write(text)
        r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.splitlines()]
        got = np.full_like(exit_, -1.0)
        for _, a, b, v in (w for w in rows if w[0] == 'exit'):
            got[int(a), int(b)] = float.fromhex(v)
        assert np.array_equal(got, exit_), (name, np.argwhere(got != exit_)[:8].tolist())                      # float64 ==: every bit (no zero has a sign here)
        zones = np.array([[float.fromhex(w[2]), float.fromhex(w[3])] for w in rows if w[0] == 'zone'])
        assert np.array_equal(zones[:, 0], zone_in) and np.array_equal(zones[:, 1], zone_out), name
        npcs = [w for w in rows if w[0] == 'npc']
        assert [int(w[1]) for w in npcs] == list(range(len(stop_at)))
        assert np.array_equal(np.array([float.fromhex(w[2]) for w in npcs]), stop_at), name
        assert [int(w[3]) for w in npcs] == yield_to.tolist(), name


def test_the_header_equals_the_model(cases, tmp_path):
    check(build('give_way_host'), cases, str(tmp_path))


def test_clean_under_the_sanitizers(cases, tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries are loaded
    program = build('give_way_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    check(program, cases, str(tmp_path))
