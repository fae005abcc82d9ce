"""
The per-row arithmetic of the route step's backward (torchdrivesim_amd/csrc/tds_route_grad.h: the clip of a segment to its piece, the foot's
gradients, a lookahead point's) compiled for the HOST by tests/route_grad_host.cpp with g++ -ffp-contract=off, fed the rows of the ring and held to
the float64 autograd model tests/route_grad_model.py.  The program is also built with the address and undefined-behaviour sanitizers and run as
it is; nothing is loaded into Python.  CPU only.

The bar: |program - model| <= 1e-12 x max(1, largest entry).  An output is a sum of at most 34 float64 terms (two of the foot, one per lookahead
point, K <= 32) of 1.1e-16 relative error each; the margin of 250 is for the order in which autograd sums them.
"""
import copy
import os
import subprocess

import numpy as np
import pytest

import route_grad_model as rgm
import route_model as rm
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'route_grad_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
F32 = np.float32


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def run(program, text):
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope='module')
def ring():
    return rm.Lanes(rm.ring_with_fork())


def ring_rows(ring):
    """(route, cursor's piece, [x, y, sin, cos], K, spacing) on the ring: interior feet on a lapping route at every lookahead count, feet clamped
    at both ends of a route that ends inside a segment, lookahead points beyond the end, a pose on a corner's diagonal"""
    for seed in range(4000):
        lap = rm.sample(ring, 0, 2.5, 200.0, seed, 0, 0)
        if lap.length == 200.0:
            break
    short = rm.sample(ring, 0, 2.5, 6.0, 1, 0, 0)
    rows = []
    for n, (q, K) in enumerate(((3.1, 0), (17.9, 16), (44.4, 32), (101.7, 5), (163.2, 32), (189.0, 16))):
        x, y = rm.point(ring, lap, q)
        rows.append((lap, q, [x + 0.3 * np.sin(n), y - 0.4 * np.cos(n), np.sin(0.3 * n + 0.1), np.cos(0.3 * n + 0.1)], K, 1.5 + n))
    rows.append((short, 0.0, [1.0, 0.4, 0.6, 0.8], 8, 1.0))                  # behind the start
    rows.append((short, 6.0, [9.75, -0.4, -0.6, 0.8], 8, 1.0))               # beyond the end
    rows.append((lap, 17.0, [21.0, -1.0, 0.0, 1.0], 4, 4.0))                 # outside corner 1, on the diagonal: the earlier segment
    return [(r, q, [float(F32(v)) for v in pose], K, float(F32(s))) for r, q, pose, K, s in rows]


def cases(ring):
    """per row: the program's input lines, and the model's four sums"""
    g = np.random.default_rng(4)
    text, want = [], []
    for route, q, pose, K, spacing in ring_rows(ring):
        r = copy.copy(route)
        r.cursor = max(j for j in range(route.n) if route.offsets[j] <= q)
        r.stored = 0.5 * q
        ch = rgm.choices(ring, r, *pose, K=K, spacing=spacing)
        grads = dict(progress=g.normal(), advance=g.normal(), remaining=g.normal(), lateral=g.normal(), heading=g.normal(size=2), lookahead=g.normal(size=(K, 2)))
        j, i = ch['piece'], ch['segment']
        c, cum = ring.cl[r.lanes[j]], ring.cum[r.lanes[j]]
        a, b = r.interval(ring, j)
        head = [c[i][0], c[i][1], c[i + 1][0], c[i + 1][1], cum[i], cum[i + 1], a, b, r.offsets[j], *pose, grads['progress'], grads['advance'],
                grads['remaining'], grads['lateral'], *grads['heading'], r.length, spacing]
        text.append(' '.join(float(v).hex() for v in head) + f' {K}')
        for m, (pj, pk, _) in enumerate(ch['look']):
            pc, pcum = ring.cl[r.lanes[pj]], ring.cum[r.lanes[pj]]
            px, py = rm.point(ring, r, ch['out']['progress'] + float(m + 1) * spacing)
            line = [px, py, float(pc[pk + 1][0]) - float(pc[pk][0]), float(pc[pk + 1][1]) - float(pc[pk][1]), pcum[pk + 1] - pcum[pk], *grads['lookahead'][m]]
            text.append(' '.join(float(v).hex() for v in line))
        want.append((ch['out']['progress'], np.concatenate(rgm.gradients(ring, r, pose[:2], pose[2:], grads, K=K, spacing=spacing)), ch))
    return '\n'.join(text) + '\n', want


@pytest.fixture(scope='module')
def output(ring):
    text, want = cases(ring)
    return run(build('route_grad_host'), text), text, want


def test_the_header_equals_the_model_on_the_rings_rows(output):
    out, _, want = output
    lines = out.splitlines()
    assert len(lines) == len(want) == 9 and all(line.startswith('row ') for line in lines)
    got = np.array([[float.fromhex(v) for v in line.split()[1:]] for line in lines])
    ref = np.array([w[1] for w in want])
    assert got[:, 0].tolist() == [w[0] for w in want], 'the progress the header recomputes is the forward\'s, bit for bit'
    bound = 1e-12 * max(1.0, float(np.abs(ref).max()))
    worst = float(np.abs(got[:, 1:] - ref).max())
    print('header against the float64 model:', worst, 'bound', bound, 'largest entry', float(np.abs(ref).max()))
    assert worst <= bound
    # the rows are what they are meant to be
    clamps = [w[2]['clamp'] for w in want]
    assert clamps == [0, 0, 0, 0, 0, 0, -1, 1, 1]
    assert any(not m for _, _, m in want[5][2]['look']) and any(m for _, _, m in want[5][2]['look']), 'lookahead on both sides of the route\'s end'
    assert (want[8][2]['piece'], want[8][2]['segment']) == (0, 3)


def test_a_segment_outside_its_piece_is_skipped():
    """the clip, on its own: a segment before the piece's interval, one without length on `cum`"""
    zeros = ' '.join(['0x0p+0'] * 13)
    rows = [f'0x0p+0 0x0p+0 0x1p+0 0x0p+0 0x0p+0 0x1p+0 0x1p+1 0x1p+2 {zeros} 0', f'0x0p+0 0x0p+0 0x1p+0 0x0p+0 0x1p+0 0x1p+0 0x0p+0 0x1p+2 {zeros} 0']
    assert run(build('route_grad_host'), '\n'.join(rows) + '\n').split() == ['skip', 'skip']


def test_clean_under_the_sanitizers(output):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    out, text, _ = output
    program = build('route_grad_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    assert run(program, text) == out
