"""
The pair test of time to collision (torchdrivesim_amd/csrc/tds_ttc.h) compiled for the HOST by tests/ttc_host.cpp: every ordered pair of the
definition cases and of random scenes, with and without a margin, within a horizon and without one, must equal the numpy model
(tests/ttc_model.py) in every bit.  The program is also built with the address and undefined-behaviour sanitizers and run as it is.  CPU only.
"""
import os
import subprocess

import numpy as np
import pytest

import ttc_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'ttc_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
NO_KEY = 0xffffffff


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def model_pairs(s, b, horizon, margin):
    """the model's verdict and time bits for every ordered pair of scene b -> (finite (E,), candidate (E,E), bits (E,E) uint32)"""
    v = tm.values(s['boxes'], s['sc'], s['speed'], b)
    E = len(v[0])
    finite = np.all([np.isfinite(q) for q in v], 0)
    safe = [np.where(finite, q, 0.0) for q in v]
    cand, bits = np.zeros((E, E), bool), np.full((E, E), NO_KEY, np.uint32)
    for a in range(E):
        c, t = tm.pair_ttc([q[a] for q in safe], safe, horizon, np.float32(margin))
        cand[a] = c
        bits[a] = np.where(c, t.view(np.uint32), NO_KEY)
    return finite, cand, bits


@pytest.fixture(scope='module')
def cases():
    """[(name, scene dict, b, horizon, margin)] and the program's input"""
    out = []
    d = tm.definition_cases()
    for b in range(2):
        out += [(f'definition {b}', d, b, tm.DEFINITION_HORIZON, 0.0), (f'definition {b} margin', d, b, float('inf'), 0.75)]
    for name in ('E6', 'E64', 'E130'):
        s, _ = tm.scenes(name)
        out += [(name, s, 0, 3.0, 0.0), (name + ' margin', s, 1, float('inf'), 0.5), (name + ' negative margin', s, 0, 5.0, -0.25)]
    text = []
    for _, s, b, horizon, margin in out:
        v = [s['boxes'][b, :, 0], s['boxes'][b, :, 1], s['boxes'][b, :, 2], s['boxes'][b, :, 3], s['sc'][b, :, 0], s['sc'][b, :, 1], s['speed'][b]]
        text.append(f'scene {len(v[0])} {float(np.float32(horizon)).hex()} {float(np.float32(margin)).hex()}')
        text += [' '.join(float(q[e]).hex() for q in v) for e in range(len(v[0]))]
    return out, '\n'.join(text) + '\n'


def check(program, cases, tmp):
    out, text = cases
    path = os.path.join(tmp, 'ttc.txt')
    with open(path, 'w') as f:
        f.write(text)
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    starts = [i for i, w in enumerate(rows) if w[0] == 'scene'] + [len(rows)]
    assert len(starts) == len(out) + 1
    candidates = zeros = 0
    for k, (name, s, b, horizon, margin) in enumerate(out):
        finite, cand, bits = model_pairs(s, b, horizon, margin)
        E = len(finite)
        part = rows[starts[k]:starts[k + 1]]
        assert int(part[0][1]) == E and [int(w[2]) for w in part if w[0] == 'finite'] == finite.astype(int).tolist(), name
        got_c, got_b = np.zeros((E, E), bool), np.full((E, E), NO_KEY, np.uint32)
        seen = np.zeros((E, E), bool)
        for _, a, e, c, t in (w for w in part if w[0] == 'pair'):
            got_c[int(a), int(e)], got_b[int(a), int(e)], seen[int(a), int(e)] = int(c), int(t, 16), True
        want_seen = finite[:, None] & finite[None, :] & ~np.eye(E, dtype=bool)
        assert np.array_equal(seen, want_seen), name
        assert np.array_equal(got_c[seen], cand[seen]), (name, np.argwhere((got_c != cand) & seen)[:8].tolist())
        assert np.array_equal(got_b[seen], bits[seen]), (name, np.argwhere((got_b != bits) & seen)[:8].tolist())
        candidates += int(cand[seen].sum())
        zeros += int((bits[seen] == 0).sum())
    assert candidates >= 100 and zeros >= 10                                                     # the comparison did not pass on empty tables


def test_the_header_equals_the_model(cases, tmp_path):
    check(build('ttc_host'), cases, str(tmp_path))


def test_clean_under_the_sanitizers(cases, tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries are loaded
    program = build('ttc_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    check(program, cases, str(tmp_path))
