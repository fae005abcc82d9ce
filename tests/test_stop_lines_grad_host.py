"""
The gradient of the stop-line observations (torchdrivesim_amd/csrc/tds_stop_lines_grad.h) compiled for the HOST by
tests/stop_lines_grad_host.cpp: an observer's four gradients must equal the float64 restatement below (`row_gradient`: the slot gradient
operation for operation, the four lanes' sums and the butterfly in the header's order) in every bit -- on the rows of random scenes at K = 1, 4, 17
and 32, on the definition cases, on an observer exactly on a line (r == 0), on empty and garbage indices and on NaN / inf incoming gradients in
empty slots.  The restatement is itself held to the autograd model (tests/stop_lines_grad_model.py).  The program is also built with the address
and undefined-behaviour sanitizers and run as it is.  CPU only.
"""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import lights_model as lm
import stop_lines_grad_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'stop_lines_grad_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
F32, F64 = np.float32, np.float64
LANES = 4               # SLG_ROW_LANES


def slot_gradient(xa, ya, s, c, xn, yn, sl, cl, g0, g1, g2, g3, g7):
    """csrc/tds_stop_lines_grad.h: stop_lines_slot_grad, operation for operation in Python floats (binary64, every operation rounded once)"""
    dx, dy = xn - xa, yn - ya
    r = math.sqrt(dx * dx + dy * dy)
    q = 0.0 if r == 0.0 else g7 / r
    return [-(g0 * c - g1 * s) - q * dx, -(g0 * s + g1 * c) - q * dy, ((g0 * dy - g1 * dx) - g2 * cl) + g3 * sl, ((g0 * dx + g1 * dy) + g2 * sl) + g3 * cl]


def row_gradient(case):
    """stop_lines_row_grad: lane l adds its filled slots l, l + 4, ... in that order to +0; then rounds m = 2, 1 of lane l + lane l ^ m; lane 0"""
    lines, observer, index, g = case
    N = len(lines)
    xa, ya, s, c = (float(v) for v in observer)
    sums = [[0.0] * 4 for _ in range(LANES)]
    for lane in range(LANES):
        for k in range(lane, len(index), LANES):
            n = int(index[k])
            if not 0 <= n < N:
                continue
            d = slot_gradient(xa, ya, s, c, *(float(v) for v in lines[n]), *(float(g[k, i]) for i in (0, 1, 2, 3, 7)))
            sums[lane] = [sums[lane][i] + d[i] for i in range(4)]
    m = LANES // 2
    while m:
        sums = [[sums[lane][i] + sums[lane ^ m][i] for i in range(4)] for lane in range(LANES)]
        m //= 2
    return sums[0]


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def rows_of(s, index, g):
    """every present observer of a scene dict as a case: (lines (N,4) [x, y, sin, cos], observer (4,), index (K,), g (K,8)), float32"""
    out = []
    for b, a in np.argwhere(s['agent_present']):
        lines = np.concatenate([s['lines'][b, :, :2], s['line_sc'][b]], -1).astype(F32)
        out.append((lines, np.concatenate([s['agent_xy'][b, a], s['agent_sc'][b, a]]).astype(F32), index[b, a].astype(np.int64), g[b, a].astype(F32)))
    return out


@pytest.fixture(scope='module')
def cases():
    rng = np.random.default_rng(71)
    out = []
    for seed, A, N, K, reach, ahead in ((1, 40, 6, 1, 80.0, True), (2, 60, 33, 4, 60.0, True), (3, 40, 33, 17, float('inf'), False), (4, 30, 40, 32, float('inf'), False)):
        s = lm.random_scenes(seed, 2, A, N)
        index = lm.stop_lines(**s, k=K, max_distance=reach, ahead_only=ahead)[1]
        g = (rng.standard_normal(index.shape + (8,)) * 10.0 ** rng.integers(-3, 4, index.shape + (1,))).astype(F32)
        g[index < 0] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1.0], F32), size=(int((index < 0).sum()), 8))        # what an empty slot holds
        g[..., 4:7] = np.where(rng.random(index.shape + (3,)) < 0.2, F32(np.nan), g[..., 4:7])                            # g4 .. g6 are never read
        out += rows_of(s, index, g)
    d = lm.definition_cases()
    d['agent_xy'] = np.nan_to_num(d['agent_xy'], nan=2.0)
    d['lines'] = np.nan_to_num(d['lines'], nan=-7.0)
    for filters, index in lm.DEFINITION_INDEX.items():
        index = np.array(index, np.int32)
        for unit in range(8):
            g = np.zeros(index.shape + (8,), F32)
            g[..., unit] = 1.0
            g[index < 0] = np.nan
            out += rows_of(d, index, g)
    # garbage: indices out of range on both sides, with NaN coming in there; the observer ON line 0 with a gradient on the distance; no lines
    lines = np.array([[1, 1, 0, 1], [4, 5, 0.6, 0.8]], F32)
    garbage = np.array([0, 2, -1, 2 ** 31 - 1, -2 ** 31, 1, 1000000, -7], np.int64)
    g = rng.standard_normal((8, 8)).astype(F32)
    g[[1, 2, 3, 4, 6, 7]] = np.nan
    out.append((lines, np.array([1, 1, 0.6, 0.8], F32), garbage, g))
    out.append((lines, np.array([1, 1, 0, 1], F32), np.array([0], np.int64), np.array([[0, 0, 0, 0, 0, 0, 0, 3.0]], F32)))
    out.append((np.zeros((0, 4), F32), np.array([1, 1, 0, 1], F32), np.array([-1, 0, 5, -1], np.int64), np.full((4, 8), np.nan, F32)))
    return out


def word(v):
    v = float(v)
    return 'nan' if math.isnan(v) else ('inf' if v > 0 else '-inf') if math.isinf(v) else v.hex()


def check(program, cases, tmp):
    path = os.path.join(tmp, 'stop_lines_grad.txt')
    with open(path, 'w') as f:
        for lines, observer, index, g in cases:
            f.write(' '.join([str(len(lines)), str(len(index))] + [word(v) for v in lines.ravel()] + [word(v) for v in observer] + [str(int(n)) for n in index] +
                             [word(v) for v in g.ravel()]) + '\n')
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases) and all(w[0] == 'row' and len(w) == 5 for w in rows)
    got_bits = np.array([[int(x, 16) for x in w[1:]] for w in rows], np.uint64)
    want = np.array([row_gradient(c) for c in cases], F64)
    bad = np.argwhere(got_bits != want.view(np.uint64))
    assert not len(bad), (bad[:8].tolist(), got_bits[bad[0][0]].view(F64).tolist(), want[bad[0][0]].tolist())
    # the comparison did not pass on empty tables
    assert len(cases) >= 400 and np.isfinite(want).all() and (np.abs(want).max(-1) > 0).sum() >= 300 and (np.abs(want).max(-1) == 0).sum() >= 10
    assert not np.signbit(want[np.abs(want).max(-1) == 0]).any(), 'a row without a filled slot is +0'
    on_line, nothing = want[-2], want[-1]
    assert not on_line.any() and not nothing.any() and want[-3].any()


def test_the_header_equals_the_restatement(cases, tmp_path):
    check(build('stop_lines_grad_host'), cases, str(tmp_path))


def test_clean_under_the_sanitizers(cases, tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error -- a
    read at a garbage index would be one"""
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries are loaded
    program = build('stop_lines_grad_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    check(program, cases, str(tmp_path))


def test_the_restatement_against_autograd(cases):
    """float64 both, other orders of operations: every row as a scene of one observer.  An entry is a sum of at most 32 slots of at most six
    products of at most some 200 |g|: 1e-11 of the row's largest |g| times 200 is far above that rounding"""
    worst = 0.0
    for lines, observer, index, g in cases:
        if not len(lines):
            continue
        full = np.concatenate([lines[:, :2], np.zeros((len(lines), 3), F32)], -1)[None]
        g_xy, g_sc, filled = gm.scene_gradients(observer[None, None, :2], observer[None, None, 2:], full, lines[None, :, 2:], index[None, None], g[None, None])
        model = np.concatenate([g_xy[0, 0], g_sc[0, 0]])
        want = np.array(row_gradient((lines, observer, index, g)))
        live = g[filled[0, 0]][:, [0, 1, 2, 3, 7]] if filled.any() else np.zeros((1, 1))
        scale = 200.0 * max(1.0, float(np.abs(live).max()))
        worst = max(worst, float(np.abs(want - model).max()) / scale)
    assert worst <= 1e-11, worst


def test_nothing_of_hip_in_the_header():
    import re
    src = re.sub(r'//.*', '', open(os.path.join(INC, 'tds_stop_lines_grad.h')).read())
    assert src.count('#define TDS_HD __host__ __device__') == 1 and '#ifdef __HIPCC__' in src          # tds_ttc.h's, for a file that stands alone
    src = src.replace('#define TDS_HD __host__ __device__', '')
    assert 'hip' not in src.lower().replace('__hipcc__', '') and '__device__' not in src and '__global__' not in src
    assert '#include' in src and 'tds_common.h' not in src and 'tds_observers.h' not in src
    assert f'constexpr int SLG_ROW_LANES = {LANES};' in src
