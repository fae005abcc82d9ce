"""
The slot gradient of the neighbour observations (torchdrivesim_amd/csrc/tds_neighbors_grad.h) compiled for the HOST by
tests/neighbors_grad_host.cpp: the 14 contributions of a slot must equal the numpy float64 restatement below (`slot_contributions`) in every bit
-- on the filled slots of the device tests' random scenes, on every ordered pair of the definition cases, and on slots whose gradient is a unit
vector or zero.  The restatement is itself held to the autograd model (tests/neighbors_grad_model.py).  The program is also built with the
address and undefined-behaviour sanitizers and run as it is.  CPU only.
"""
import os
import subprocess

import numpy as np
import pytest

import neighbors_grad_model as gm
import neighbors_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'neighbors_grad_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
F32, F64 = np.float32, np.float64


def slot_contributions(v):
    """csrc/tds_neighbors_grad.h restated, operation for operation in the header's order: v (n, 18) float32 -- x y sin cos speed of the observer,
    of the entity, g0 .. g7 -> (n, 14) float64, the observer's seven [x, y, length, width, sin, cos, speed] first"""
    v = np.asarray(v, F32).astype(F64)
    xa, ya, s, c, va, xe, ye, se, ce, ve = v[:, :10].T
    g = v[:, 10:].T
    dx, dy = xe - xa, ye - ya
    f2, f3 = se * c - ce * s, ce * c + se * s
    G2, G3 = g[2] + g[5] * ve, g[3] + g[4] * ve
    px, py = g[0] * c - g[1] * s, g[0] * s + g[1] * c
    zero = np.zeros(len(v))
    ga = [-px, -py, zero, zero, ((g[0] * dy - g[1] * dx) - G2 * ce) + G3 * se, ((g[0] * dx + g[1] * dy) + G2 * se) + G3 * ce, -g[4]]
    ge = [px, py, g[6], g[7], G2 * c + G3 * s, G3 * c - G2 * s, g[4] * f3 + g[5] * f2]
    return np.stack(ga + ge, -1)


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def slots_of(s, b, a, e, g):
    pose = lambda i: np.concatenate([s['boxes'][b, i, :2], s['sc'][b, i], s['speed'][b, i, None]], -1)
    return np.concatenate([pose(a), pose(e), g], -1).astype(F32)


@pytest.fixture(scope='module')
def cases():
    """(n, 18) float32: the filled slots of four of the device tests' scenes with random gradients, every ordered pair of the finite entities of
    the definition cases with unit gradients on each feature and with none"""
    rng = np.random.default_rng(18)
    parts = []
    for name in ('E6', 'E64', 'E33', 'E130'):
        seed, B, A, E, K, reach = gm.CASES[name]
        s = nm.random_scenes(seed, B, A, E)
        index = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], A, K, reach)[1]
        _, b, a, k, e = gm.filled_slots(index, E)
        parts.append(slots_of(s, b, a, e, rng.standard_normal((len(b), 8)) * 10.0 ** rng.integers(-3, 4, (len(b), 1))))
    d = nm.definition_cases()
    units = np.concatenate([np.eye(8), -np.eye(8), np.zeros((1, 8))]).astype(F32)
    for b in (0, 1):
        ok = np.nonzero(np.isfinite(d['boxes'][b]).all(-1))[0]
        a, e, u = (q.ravel() for q in np.meshgrid(ok, ok, np.arange(len(units)), indexing='ij'))
        keep = a != e
        parts.append(slots_of(d, np.full(keep.sum(), b), a[keep], e[keep], units[u[keep]]))
    return np.concatenate(parts)


def check(program, cases, tmp):
    path = os.path.join(tmp, 'neighbors_grad.txt')
    with open(path, 'w') as f:
        for row in cases:
            f.write(' '.join(float(v).hex() for v in row) + '\n')
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases) and all(w[0] == 'slot' and len(w) == 15 for w in rows)
    got_bits = np.array([[int(x, 16) for x in w[1:]] for w in rows], np.uint64)
    want = slot_contributions(cases)
    bad = np.argwhere(got_bits != want.view(np.uint64))
    assert not len(bad), (bad[:8].tolist(), got_bits[bad[0][0]].view(F64).tolist(), want[bad[0][0]].tolist())
    # the comparison did not pass on empty tables
    assert len(cases) >= 1500 and np.isfinite(want).all() and (np.abs(want).max(-1) > 0).sum() >= 1500 and (np.abs(want).max(-1) == 0).sum() >= 10


def test_the_header_equals_the_restatement(cases, tmp_path):
    check(build('neighbors_grad_host'), cases, str(tmp_path))


def test_clean_under_the_sanitizers(cases, tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries are loaded
    program = build('neighbors_grad_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    check(program, cases, str(tmp_path))


def test_the_restatement_against_autograd(cases):
    """float64 both, other orders of operations: every slot as a scene of two entities.  A contribution is a sum of at most six products of
    at most some 200 |g|: 1e-12 of the slot's largest contribution, or of |g|, is a hundred times that rounding"""
    v = cases.astype(F64)
    n = len(v)
    boxes = np.zeros((n, 2, 5))
    boxes[:, 0, :2], boxes[:, 1, :2] = v[:, 0:2], v[:, 5:7]
    sc = np.stack([v[:, 2:4], v[:, 7:9]], 1)
    speed = np.stack([v[:, 4], v[:, 9]], 1)
    gb, gsc, gv, filled = gm.scene_gradients(boxes, sc, speed, np.ones((n, 1, 1), np.int32), v[:, None, None, 10:])
    model = np.concatenate([gb[..., :4], gsc, gv[..., None]], -1).reshape(n, 14)
    want = slot_contributions(cases)
    scale = np.maximum(np.abs(model).max(-1, keepdims=True), np.abs(v[:, 10:]).max(-1, keepdims=True))
    assert filled.all() and (np.abs(want - model) <= 1e-12 * np.maximum(scale, 1e-300)).all()


def test_nothing_of_hip_in_the_header():
    import re
    src = re.sub(r'//.*', '', open(os.path.join(INC, 'tds_neighbors_grad.h')).read())
    assert src.count('#define TDS_HD __host__ __device__') == 1 and '#ifdef __HIPCC__' in src          # tds_ttc.h's, for a file that stands alone
    src = src.replace('#define TDS_HD __host__ __device__', '')
    assert 'hip' not in src.lower().replace('__hipcc__', '') and '__device__' not in src and '__global__' not in src
    assert '#include' in src and 'tds_common.h' not in src and 'tds_observers.h' not in src
