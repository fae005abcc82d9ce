"""
The gradients of the lane observations (torchdrivesim_amd/csrc/tds_lane_obs_grad.h) compiled for the HOST by tests/lane_obs_grad_host.cpp: the
contributions of a slot's features and of a polyline point must equal the numpy float64 restatement below (`slot_contributions`,
`point_contributions`) in every bit -- on the filled slots and valid points of the synthetic maps of tests/lane_obs_cases.py seen from their hand
poses and from random ones, with random gradients, unit gradients and none.  The restatement is itself held to the autograd model
(tests/lane_obs_grad_model.py), observer by observer.  The program is also built with the address and undefined-behaviour sanitizers and run as
it is.  CPU only.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lane_obs_cases as cases
import lane_obs_grad_model as gm
import lane_obs_model as lom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'lane_obs_grad_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
F32, F64 = np.float32, np.float64
K, P, SPACING, REACH = 4, 5, 4.0, 12.0


def slot_contributions(v):
    """tds::segment_foot, tds::segment_unit and tds::lane_obs_slot_grad restated, operation for operation in the headers' order: v (n, 20) float64
    -- the two points of the segment (x y z each), cum0, cum1, x y sin cos of the observer, g0 .. g7 -> (n, 6): x, y, sin, cos and the slide"""
    v = np.asarray(v, F64)
    ax, ay, bx, by, cum0, cum1, x, y, s, c = (v[:, i] for i in (0, 1, 3, 4, 6, 7, 8, 9, 10, 11))
    g = v[:, 12:].T
    with np.errstate(all='ignore'):
        dx, dy = bx - ax, by - ay
        l2 = dx * dx + dy * dy
        u0 = np.where(l2 > 0, ((x - ax) * dx + (y - ay) * dy) / l2, 0.0)
        u = np.fmin(np.fmax(u0, 0.0), 1.0)
        fx, fy = ax + u * dx - x, ay + u * dy - y
        d2 = fx * fx + fy * fy
        ln = np.sqrt(l2)
        tx, ty = np.where(ln > 0, dx / ln, 0.0), np.where(ln > 0, dy / ln, 0.0)
        W = cum1 - cum0
        m = (l2 > 0) & (u0 > 0.0) & (u0 < 1.0)
        sx, sy = np.where(m, (W * dx) / l2, 0.0), np.where(m, (W * dy) / l2, 0.0)
        qx, qy = g[0] * c - g[1] * s, g[0] * s + g[1] * c
        tq = tx * qx + ty * qy
        px, py = np.where(m, tq * tx - qx, -qx), np.where(m, tq * ty - qy, -qy)
        G = g[4] - g[5]
        px, py = px + G * sx, py + G * sy
        px, py = px - g[6] * ty, py + g[6] * tx
        dist = np.sqrt(d2)
        px, py = np.where(dist > 0.0, px - g[7] * (fx / dist), px), np.where(dist > 0.0, py - g[7] * (fy / dist), py)
        gs = (g[0] * fy - g[1] * fx) + (g[3] * ty - g[2] * tx)
        gc = (g[0] * fx + g[1] * fy) + (g[2] * ty + g[3] * tx)
    return np.stack([px, py, gs, gc, sx, sy], -1)


def foot_u(v):
    """the clamped u of `slot_contributions`' rows"""
    ax, ay, bx, by, x, y = (np.asarray(v, F64)[:, i] for i in (0, 1, 3, 4, 8, 9))
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    with np.errstate(all='ignore'):
        return np.fmin(np.fmax(np.where(l2 > 0, ((x - ax) * dx + (y - ay) * dy) / l2, 0.0), 0.0), 1.0)


def point_contributions(v):
    """tds::lane_obs_point_grad restated: v (n, 10) float64 -- the slide, ex ey hx hy, sin cos, gx gy -> (n, 4)"""
    sx, sy, ex, ey, hx, hy, s, c, gx, gy = np.asarray(v, F64).T
    rx, ry = gx * c - gy * s, gx * s + gy * c
    hr = hx * rx + hy * ry
    return np.stack([hr * sx - rx, hr * sy - ry, gx * ey - gy * ex, gx * ex + gy * ey], -1)


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def observers():
    """(lanes, pose (4,) float32, index (K,)) of every map's hand poses (psi as [sin, cos]) and 12 random ones"""
    for name, make in dict(cases.STRUCTURES, ring=cases.ring).items():
        m = make()
        lanes = lom.Lanes(m)
        rng = np.random.default_rng(len(name))
        for x, y, psi in list(cases.HAND_POSES) + cases.poses(rng, m, 12).tolist():
            pose = np.array([x, y, np.sin(psi), np.cos(psi)], F32)
            yield lanes, pose, lom.observe(lanes, pose, True, K, P, SPACING, REACH)[3]


@pytest.fixture(scope='module')
def drawn():
    """the slots and points of `observers` with a gradient each -> slots (n, 20), points (n', 10) float64, and per observer what the autograd model
    needs with the rows of its slots and points"""
    rng = np.random.default_rng(21)
    units = np.concatenate([np.eye(8), -np.eye(8), np.zeros((1, 8))])
    slots, points, per_observer = [], [], []
    for lanes, pose, index in observers():
        x, y, s, c = (float(v) for v in pose)
        gf = (rng.standard_normal((K, 8)) * 10.0 ** rng.integers(-3, 4, (K, 1))).astype(F32)
        gp = (rng.standard_normal((K, P, 2)) * 10.0 ** rng.integers(-3, 4, (K, 1, 1))).astype(F32)
        if len(per_observer) % 3 == 0:
            gf[:] = units[rng.integers(0, len(units), K)]
        mine = dict(lanes=lanes, pose=pose, index=index, gf=gf, gp=gp, slots=[], points=[])
        for k, ch in enumerate(gm.choices(lanes, pose, index, P, SPACING)):
            if ch is None:
                continue
            l, sb = ch['l'], ch['sb']
            cum = lanes.cum[l]
            mine['slots'].append(len(slots))
            slots.append(np.concatenate([lanes.cl[l][sb], lanes.cl[l][sb + 1], [cum[sb], cum[sb + 1], x, y, s, c], gf[k].astype(F64)]))
            slide = slot_contributions(slots[-1][None])[0, 4:]
            arc = cum[sb] + ch['u'] * (cum[sb + 1] - cum[sb])
            for j, at in enumerate(ch['points']):
                if at is None:
                    continue
                cur, seg, base = at
                wx, wy, seg2, _ = lom.point_at(lanes, cur, (arc + float(j) * SPACING) - base)
                assert seg2 == seg
                a, b, w = lanes.cl[cur][seg], lanes.cl[cur][seg + 1], lanes.cum[cur][seg + 1] - lanes.cum[cur][seg]
                h = ((b[0] - a[0]) / w, (b[1] - a[1]) / w) if w > 0 else (0.0, 0.0)
                mine['points'].append(len(points))
                points.append([slide[0], slide[1], wx - x, wy - y, h[0], h[1], s, c, float(gp[k, j, 0]), float(gp[k, j, 1])])
        per_observer.append(mine)
    return np.array(slots, F64), np.array(points, F64), per_observer


def check(program, slots, points, tmp):
    path = os.path.join(tmp, 'lane_obs_grad.txt')
    with open(path, 'w') as f:
        for kind, rows in (('S', slots), ('P', points)):
            for row in rows:
                f.write(kind + ' ' + ' '.join(float(v).hex() for v in row) + '\n')
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(slots) + len(points)
    for what, width, lines, want in (('slot', 6, rows[:len(slots)], slot_contributions(slots)), ('point', 4, rows[len(slots):], point_contributions(points))):
        assert all(w[0] == what and len(w) == width + 1 for w in lines)
        got_bits = np.array([[int(x, 16) for x in w[1:]] for w in lines], np.uint64)
        bad = np.argwhere(got_bits != want.view(np.uint64))
        assert not len(bad), (what, bad[:8].tolist(), got_bits[bad[0][0]].view(F64).tolist(), want[bad[0][0]].tolist())
        assert np.isfinite(want).all() and (np.abs(want[:, :4]).max(-1) > 0).sum() >= 0.9 * len(want)
    # the comparison did not pass on empty tables, and both sides of the clamp are met
    slide = slot_contributions(slots)[:, 4:]
    assert len(slots) >= 250 and len(points) >= 700 and (np.abs(slide).max(-1) > 0).sum() >= 50 and (np.abs(slide).max(-1) == 0).sum() >= 50


def test_the_header_equals_the_restatement(drawn, tmp_path):
    check(build('lane_obs_grad_host'), drawn[0], drawn[1], str(tmp_path))


def test_clean_under_the_sanitizers(drawn, tmp_path):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries are loaded
    program = build('lane_obs_grad_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    check(program, drawn[0], drawn[1], str(tmp_path))


def test_the_restatement_against_autograd(drawn):
    """float64 both, other orders of operations: per observer the sum of the restated contributions of its slots and points against the model's
    gradient.  A contribution is a handful of products of at most some 50 m |g|, an observer has at most 4 + 20 of them: 1e-11 of the largest
    entry is a thousand times that rounding.  One term is not that well determined in either: the foot offset f is a difference of coordinates of
    tens of metres, known to some 1e-15 m, so its direction f / distance -- what feature 7 passes on -- is known to 1e-15 / distance, which shows
    for the poses that lie on a centre-line point but for their rounding to float32 (distance 1e-8 .. 1e-7); 1e-13 |g7| / distance is allowed"""
    slots, points, per_observer = drawn
    sc, pc = slot_contributions(slots)[:, :4], point_contributions(points)
    held = 0
    for o in per_observer:
        pose = o['pose']
        g_xy, g_sc, filled, valid = gm.gradients([o['lanes']], pose[None, None, :2], pose[None, None, 2:], o['index'][None, None], o['gf'][None, None],
                                                 o['gp'][None, None], P, SPACING)
        assert filled.sum() == len(o['slots']) and valid.sum() == len(o['points'])
        want = np.concatenate([g_xy[0, 0], g_sc[0, 0]])
        got = sc[o['slots']].sum(0) + pc[o['points']].sum(0)
        scale = max(1.0, np.abs(want).max(), np.abs(sc[o['slots']]).max(initial=0.0), np.abs(pc[o['points']]).max(initial=0.0))
        rows = slots[o['slots']]
        dist = np.sqrt(((rows[:, 0] + foot_u(rows) * (rows[:, 3] - rows[:, 0]) - rows[:, 8]) ** 2 + (rows[:, 1] + foot_u(rows) * (rows[:, 4] - rows[:, 1]) - rows[:, 9]) ** 2))
        loose = float((1e-13 * np.abs(rows[:, 19])[dist > 0] / dist[dist > 0]).sum())
        assert np.abs(got - want).max() <= 1e-11 * scale + loose, (pose.tolist(), got.tolist(), want.tolist())
        held += len(o['slots']) > 0
    assert held >= 80


def test_nothing_of_hip_in_the_header():
    src = re.sub(r'//.*', '', open(os.path.join(INC, 'tds_lane_obs_grad.h')).read())
    assert 'hip' not in src.lower() and '__device__' not in src and '__global__' not in src and 'atomic' not in src and 'asm' not in src
    assert '#include "tds_lane_math.h"' in src and 'tds_common.h' not in src and 'tds_lanes.h' not in src and 'tds_lane_obs.h' not in src
