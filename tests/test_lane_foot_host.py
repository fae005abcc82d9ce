"""
The foot of a pose on a centre-line segment -- tds::segment_foot and what is read off it (torchdrivesim_amd/csrc/tds_lane_math.h), the one
helper tds_lane_snap and the lane observations (K8) rank a lanelet's segments by -- compiled for the HOST by tests/lane_foot_host.cpp and held
bit for bit to tests/lane_obs_model.py, the float64 model the K8 kernel is compared with on the GPU, and to the foot of
tests/lane_follow_model.py, the model of tds_lane_snap.  The program is also built with the address and undefined-behaviour sanitizers and run
as it is.  CPU only.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import lane_follow_model as lfm
import lane_obs_model as lom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'lane_foot_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
N_POINTS, N_POSES = 6, 16


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def run(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope='module')
def output():
    return run(build('lane_foot_host'))


def rows(output, tag):
    return [line.split()[1:] for line in output.splitlines() if line.startswith(tag + ' ')]


def same(a, b):
    """equal as IEEE doubles, the sign of a zero included; a NaN equals a NaN"""
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


@pytest.fixture(scope='module')
def line(output):
    pts = np.array([[float.fromhex(v) for v in r] for r in rows(output, 'point')])
    assert pts.shape == (N_POINTS, 4)

    class _Lanelet:
        centerline = pts[:, :3]
        attributes, left_ids, right_ids = {}, [], []

        def polygon2d(self):
            return self.centerline[:, :2]

    class _Map:
        laneletLayer = [_Lanelet()]
    lanes = lfm.Lanes(_Map())
    assert all(same(a, b) for a, b in zip(lanes.cum[0], pts[:, 3]))          # the program summed the lengths as the table does
    return lanes


def feet_rows(output):
    return [([float.fromhex(v) for v in r[:2]], int(r[2]), [float.fromhex(v) for v in r[3:]]) for r in rows(output, 'foot')]


def test_the_helper_equals_the_model_on_every_recorded_segment(output, line):
    got = feet_rows(output)
    assert len(got) == N_POSES * (N_POINTS - 1)
    c, cum = line.cl[0], line.cum[0]
    seen_zero_length = seen_clamped = seen_inside = False
    for (x, y), i, vals in got:
        ax, ay, dx, dy, l2, u, fx, fy, d2 = lom.segment_foot(c, i, x, y)
        ln = math.sqrt(l2)
        tx, ty = (dx / ln, dy / ln) if ln > 0 else (0.0, 0.0)
        want = [ax, ay, dx, dy, l2, u, fx, fy, d2, tx, ty, cum[i] + u * (cum[i + 1] - cum[i]), tx * (y - ay) - ty * (x - ax)]
        assert all(same(g, w) for g, w in zip(vals, want)), ((x, y), i, vals, want)
        assert 0.0 <= vals[5] <= 1.0                                            # u is never a NaN, whatever the pose
        seen_zero_length |= l2 == 0.0 and u == 0.0 and tx == 0.0
        seen_clamped |= u in (0.0, 1.0) and l2 > 0.0
        seen_inside |= 0.0 < u < 1.0
    assert seen_zero_length and seen_clamped and seen_inside


def test_the_vectorised_model_equals_the_scalar_one_and_the_snap_model(output, line):
    """`lane_obs_model.feet` (all segments of a lanelet at once) picks the segment and the d2 the scalar loop over the helper's rows picks, and
    for finite poses that is the foot of tests/lane_follow_model.py, the model of tds_lane_snap"""
    got = feet_rows(output)
    c = line.cl[0]
    for p in range(N_POSES):
        block = got[p * (N_POINTS - 1):(p + 1) * (N_POINTS - 1)]
        (x, y) = block[0][0]
        best, sb = math.inf, -1
        for _, i, vals in block:
            if vals[8] < best:
                best, sb = vals[8], i
        d2, seg = lom.feet(line, x, y)
        assert int(seg[0]) == sb and (sb < 0 or same(float(d2[0]), best)), (x, y)
        if math.isfinite(x) and math.isfinite(y):
            k, u, tx, ty = lfm.foot(c, x, y)
            assert k == sb and same(u, block[sb][2][5]) and same(tx, block[sb][2][9]) and same(ty, block[sb][2][10])
        else:
            assert sb == -1                                                      # no d2 below +inf: no candidate


def test_clean_under_the_sanitizers(output):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    program = build('lane_foot_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    assert run(program) == output
