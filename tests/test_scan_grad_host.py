"""
The per-ray arithmetic of the range scans and of their backward (torchdrivesim_amd/csrc/tds_scan.h, tds_scan_grad.h) compiled for the HOST by
tests/scan_grad_host.cpp: the slab test with the slab that binds, the ten derivatives of the agent part, the edge a road stretch ends on (the
candidates and the tie rule) and the four derivatives of the road part must equal the numpy restatement below in every bit.  The restatement is
itself held to the autograd model (tests/range_scan_grad_model.py).  The program is also built with the address and undefined-behaviour
sanitizers and run as it is.  CPU only.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import range_scan_grad_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'scan_grad_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
F32, F64 = np.float32, np.float64
INF32 = F32(np.inf)


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def slab_test(lx, ly, ex, ey, hl, hw):
    """tds_scan.h slab_test, float32 scalars -> (ok, t0, slab)"""
    t0, t1, ok, slab = F32(0), INF32, True, 0
    for k, (l, e, h) in enumerate(((lx, ex, hl), (ly, ey, hw))):
        if e == 0:
            ok = ok and abs(l) <= h
        else:
            u, v = (-h - l) / e, (h - l) / e
            if min(u, v) > t0:
                slab = k + 1
            t0, t1 = max(t0, min(u, v)), min(t1, max(u, v))
    return bool(ok and t0 <= t1), t0, slab


def agent_case(v):
    """one 'a' line (10 float32) -> (ok, t0, slab, the ten float64 derivatives), operation for operation in the headers' order"""
    ox, oy, cx, cy, length, width, s, c, dx, dy = (F32(x) for x in v)
    hl, hw = length / F32(2), width / F32(2)
    rx, ry = ox - cx, oy - cy
    lx, ly = rx * c + ry * s, ry * c - rx * s
    ex, ey = dx * c + dy * s, dy * c - dx * s
    ok, t0, slab = slab_test(lx, ly, ex, ey, hl, hw)
    g = np.zeros(10)
    if ok and slab:
        xs = slab == 1
        e32 = ex if xs else ey
        rx, ry = F64(ox) - F64(cx), F64(oy) - F64(cy)
        s, c, dx, dy = F64(s), F64(c), F64(dx), F64(dy)
        l = rx * c + ry * s if xs else ry * c - rx * s
        e = dx * c + dy * s if xs else dy * c - dx * s
        h = F64(hl) if xs else F64(hw)
        sigma = -1.0 if e32 > 0 else 1.0
        t = (sigma * h - l) / e
        tl, th, te = -1.0 / e, sigma / e, -t / e
        l_rx, l_ry, l_s, l_c = (c, s, ry, rx) if xs else (-s, c, -rx, ry)
        e_dx, e_dy, e_s, e_c = (c, s, dy, dx) if xs else (-s, c, -dx, dy)
        g[:] = [tl * l_rx, tl * l_ry, -(tl * l_rx), -(tl * l_ry), th * 0.5 if xs else 0.0, 0.0 if xs else th * 0.5, tl * l_s + te * e_s,
                tl * l_c + te * e_c, te * e_dx, te * e_dy]
    return ok, t0, slab, g


def crossing(wi, wj, ui, uj):
    if wi != wj and min(wi, wj) <= 0 and max(wi, wj) >= 0:
        return ui + (uj - ui) * (wi / (wi - wj))
    return None


def face_hi(o, d, f):
    """tds_scan.h line_triangle on a face (6 float32, world) -> (hi or None, the crossings of its three edges)"""
    ox, oy, dx, dy = (F32(x) for x in (*o, *d))
    p = [(F32(f[2 * i]) - ox, F32(f[2 * i + 1]) - oy) for i in range(3)]
    w = [dx * q[1] - dy * q[0] for q in p]
    if all(x > 0 for x in w) or all(x < 0 for x in w):
        return None, [None] * 3
    u = [dx * q[0] + dy * q[1] for q in p]
    cr = [crossing(w[i], w[j], u[i], u[j]) for i, j in ((0, 1), (1, 2), (2, 0))]
    have = [x for x in cr if x is not None]
    if not have or not min(have) <= max(have):
        return None, cr
    return max(have), cr


def positive_area(f):
    x0, y0, x1, y1, x2, y2 = (F64(F32(x)) for x in f)
    return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0) != 0.0


def road_case(o, d, F, faces):
    """one 'r' line -> (found, the oriented edge (4 float32), the four float64 derivatives)"""
    best = None
    for f in faces:
        hi, cr = face_hi(o, d, f)
        if hi is None or hi != F or not positive_area(f):
            continue
        for (i, j), u in zip(((0, 1), (1, 2), (2, 0)), cr):
            if u is not None and u == F:
                e = gm.oriented((F32(f[2 * i]), F32(f[2 * i + 1])), (F32(f[2 * j]), F32(f[2 * j + 1])))
                best = e if best is None or e < best else best
    g = np.zeros(4)
    if best is not None:
        ox, oy, dx, dy = (F64(F32(x)) for x in (*o, *d))
        pix, piy, pjx, pjy = F64(best[0]) - ox, F64(best[1]) - oy, F64(best[2]) - ox, F64(best[3]) - oy
        ui, uj = dx * pix + dy * piy, dx * pjx + dy * pjy
        wi, wj = dx * piy - dy * pix, dx * pjy - dy * pjx
        D, du = wi - wj, uj - ui
        lam, q = wi / D, du / D
        twi, twj = -(q * wj) / D, (q * wi) / D
        g[:] = [dy * q - dx, -(dx * q) - dy, ((pix + lam * (pjx - pix)) + twi * piy) + twj * pjy, ((piy + lam * (pjy - piy)) - twi * pix) - twj * pjx]
    return best is not None, np.array(best if best is not None else (0, 0, 0, 0), F32), g


# ------------------------------------------------------------------------------------------------------------------------ the cases
@pytest.fixture(scope='module')
def agent_cases():
    """rays of random scenes against every other rectangle; rays parallel to a side (e == 0), from inside, and square on a face"""
    rows = []
    for seed in (1, 2, 3):
        s = gm.random_boxes(seed, 1, 4, 12, spread=15.0, absent=0.0)
        rays = gm.rays_of(s['boxes'], 4, 16)
        for a in range(4):
            for j in range(12):
                if j != a:
                    for k in range(16):
                        rows.append([*s['boxes'][0, a, :2], *s['boxes'][0, j, :4], *s['sc'][0, j], rays[0, a, k, 1], rays[0, a, k, 0]])
    for ox, oy, dx, dy in ((-10, 0, 1, 0), (-10, 0.5, 1, 0), (-10, 3, 1, 0), (0, -7, 0, 1), (0.5, 0.2, 1, 0), (0.5, 0.2, 0.6, 0.8), (10, 0, -1, 0),
                           (-10, -10, 0.6, 0.8), (3, 9, 0, -1), (2, 1, 1, 0), (-2, -1, 1, 0)):
        rows.append([ox, oy, 0, 0, 4, 2, 0, 1, dx, dy])
        rows.append([ox, oy, 0, 0, 4, 2, 1, 0, dx, dy])
    return np.array(rows, F32)


@pytest.fixture(scope='module')
def road_cases():
    """a strip of triangulated quads with jittered vertices, a padding face and a repeated face; origins inside it; every ray with the stretch
    to the far end of each face its line meets -- shared edges give two candidates with the same end points"""
    g = np.random.default_rng(7)
    xs = np.arange(0, 40, 5.0)
    lower = np.stack([xs, g.uniform(-0.3, 0.3, len(xs))], -1).astype(F32)
    upper = np.stack([xs + g.uniform(-1, 1, len(xs)), 6 + g.uniform(-0.3, 0.3, len(xs))], -1).astype(F32)
    faces = []
    for i in range(len(xs) - 1):
        faces.append([*lower[i], *lower[i + 1], *upper[i + 1]])
        faces.append([*lower[i], *upper[i + 1], *upper[i]])
    faces.append([0, 0, 0, 0, 0, 0])
    faces.append(faces[3])
    faces.append([*lower[0], *lower[1], *(2 * lower[1] - lower[0])])          # a sliver: three points in a line
    faces = np.array(faces, F32)
    cases = []
    for _ in range(40):
        o = np.array([g.uniform(3, 32), g.uniform(1.5, 4.5)], F32)
        for k in range(16):
            ang = F32(g.uniform(-np.pi, np.pi))
            d = (np.cos(ang, dtype=F32), np.sin(ang, dtype=F32))
            his = sorted({float(h) for h in (face_hi(o, d, f)[0] for f in faces) if h is not None and h > 0})
            for F in his[:3]:
                cases.append((o, d, F32(F), faces))
    cases.append((np.array([5, 3], F32), (F32(1), F32(0)), F32(123.0), faces))                 # no face ends there
    return cases


def write_cases(path, agent_cases, road_cases):
    hx = lambda v: float(v).hex()
    with open(path, 'w') as f:
        for row in agent_cases:
            f.write('a ' + ' '.join(hx(v) for v in row) + '\n')
        for o, d, F, faces in road_cases:
            f.write('r ' + ' '.join(hx(v) for v in (*o, *d, F, len(faces), *faces.ravel())) + '\n')


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def check(program, agent_cases, road_cases, tmp):
    path = os.path.join(tmp, 'scan_grad.txt')
    write_cases(path, agent_cases, road_cases)
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(agent_cases) + len(road_cases)
    bits64 = lambda words: np.array([int(x, 16) for x in words], np.uint64).view(F64)
    slabs = np.zeros(3, int)
    for w, v in zip(rows, agent_cases):
        ok, t0, slab, g = agent_case(v)
        assert w[0] == 'a' and len(w) == 14
        got = (int(w[1]), int(w[2], 16), int(w[3]))
        assert got == (int(ok), int(np.array(t0, F32).view(np.uint32)), slab), (v.tolist(), got, ok, t0, slab)
        assert np.array_equal(bits64(w[4:]).view(np.uint64), g.view(np.uint64)), (v.tolist(), bits64(w[4:]).tolist(), g.tolist())
        slabs[slab] += ok
    found = 0
    for w, (o, d, F, faces) in zip(rows[len(agent_cases):], road_cases):
        ok, edge, g = road_case(o, d, F, faces)
        assert w[0] == 'r' and len(w) == 10 and int(w[1]) == int(ok), (o, d, F)
        if ok:
            assert [int(x, 16) for x in w[2:6]] == edge.view(np.uint32).tolist(), (o, d, F, edge)
        assert np.array_equal(bits64(w[6:]).view(np.uint64), g.view(np.uint64)), (o, d, F, bits64(w[6:]).tolist(), g.tolist())
        found += ok
    # the comparison did not pass on empty tables
    assert slabs.min() >= 10 and found >= 500 and found < len(road_cases), (slabs, found)


def test_the_headers_equal_the_restatement(agent_cases, road_cases, tmp_path):
    check(build('scan_grad_host'), agent_cases, road_cases, str(tmp_path))


def test_clean_under_the_sanitizers(agent_cases, road_cases, tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    program = build('scan_grad_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    check(program, agent_cases, road_cases, str(tmp_path))


def test_the_restatement_against_autograd(agent_cases, road_cases):
    """float64 both, other orders of operations: every case as a scene of its own.  A derivative is a handful of products and quotients of
    numbers up to some 1e3 / |e|: 1e-10 of the case's largest derivative is far above that rounding and far below any wrong term"""
    rows = [(v, agent_case(v)) for v in agent_cases]
    rows = [(v, slab, g) for v, (ok, _, slab, g) in rows if ok and slab]
    n = len(rows)
    v = np.array([r[0] for r in rows], F64)
    boxes = np.zeros((n, 2, 5))
    boxes[:, 0, :2], boxes[:, 1, :4] = v[:, 0:2], v[:, 2:6]
    sc = np.zeros((n, 2, 2))
    sc[:, 1] = v[:, 6:8]
    ray_sc = v[:, None, None, [9, 8]]
    choice = np.array([[[[1, r[1]]]] for r in rows])
    gb, gsc, gr, la, _ = gm.scene_gradients(boxes, sc, ray_sc, choice, np.full((n, 1, 1, 4), np.nan), np.ones((n, 1, 1)), None)
    model = np.concatenate([gb[:, 0, :2], gb[:, 1, :4], gsc[:, 1], gr[:, 0, 0, ::-1]], -1)
    want = np.array([r[2] for r in rows])
    assert la.all() and n >= 100 and (np.abs(want - model) <= 1e-10 * np.abs(want).max(-1, keepdims=True)).all()
    rows = [(c, road_case(*c)) for c in road_cases]
    rows = [(c, edge, g) for c, (ok, edge, g) in rows if ok]
    n = len(rows)
    boxes = np.zeros((n, 1, 5))
    boxes[:, 0, :2] = [c[0] for c, _, _ in rows]
    ray_sc = np.array([[[[c[1][1], c[1][0]]]] for c, _, _ in rows], F64)
    edges = np.array([e for _, e, _ in rows], F64)[:, None, None]
    gb, gsc, gr, _, lr = gm.scene_gradients(boxes, np.zeros((n, 1, 2)), ray_sc, np.full((n, 1, 1, 2), -1), edges, None, np.ones((n, 1, 1)))
    model = np.concatenate([gb[:, 0, :2], gr[:, 0, 0, ::-1]], -1)
    want = np.array([g for _, _, g in rows])
    assert lr.all() and n >= 500 and (np.abs(want - model) <= 1e-10 * np.abs(want).max(-1, keepdims=True)).all() and not gsc.any()


def test_nothing_of_hip_in_the_headers():
    import re
    for name in ('tds_scan.h', 'tds_scan_grad.h'):
        src = re.sub(r'//.*', '', open(os.path.join(INC, name)).read())
        src = src.replace('#define TDS_HD __host__ __device__', '')
        assert 'hip' not in src.lower().replace('__hipcc__', '') and '__device__' not in src and '__global__' not in src, name
        assert '#include' in src and 'tds_common.h' not in src, name
