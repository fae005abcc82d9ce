"""
The arithmetic the lane kernels share (torchdrivesim_amd/csrc/tds_lane_math.h: Philox4x32-10, the scaled pick, the segment search, the point
at an arc length) compiled for the HOST by tests/lane_math_host.cpp and held to the published known answers and to the float64 models the
kernels are compared with on the GPU.  The program is also built with the address and undefined-behaviour sanitizers and run as it is.
CPU only.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import lane_follow_model as lfm
import spawn_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'lane_math_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')

ONES = 0xFFFFFFFF
KNOWN = [(((0,) * 4, (0, 0)), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),                      # Random123 kat_vectors, as tests/test_spawn_model.py
         (((ONES,) * 4, (ONES, ONES)), '408f276d 41c83b0e a20bc7c6 6d5451fd'),
         (((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
POINTS = [(-0.0, 0.0, 0.0), (-3.0, 4.0, 0.0), (-3.0, 4.0, 0.0), (-1.0, 10.0, 1.0), (-1.0, 12.0, 1.0)]


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
    return run(build('lane_math_host'))


def rows(output, tag):
    return [line.split()[1:] for line in output.splitlines() if line.startswith(tag + ' ')]


class _Lanelet:
    centerline = np.asarray(POINTS, np.float64)
    attributes, left_ids, right_ids = {}, [], []

    def polygon2d(self):
        return self.centerline[:, :2]


class _Map:
    laneletLayer = [_Lanelet()]


@pytest.fixture(scope='module')
def lanes():
    return lfm.Lanes(_Map())


def bits32(x):
    return np.float32(x).view(np.uint32)


def same(a, b):
    """equal as IEEE doubles, the sign of a zero included; a NaN equals a NaN"""
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def test_philox_known_answers(output):
    got = rows(output, 'philox')
    assert len(got) == len(KNOWN)
    for words, ((counter, key), want) in zip(got, KNOWN):
        assert words == want.split()
        assert tuple(int(w, 16) for w in words) == tuple(sm.philox4x32_10(counter, key)) == tuple(lfm.philox4x32_10(counter, key))


def test_pick_is_the_word_scaled_to_the_count(output):
    got = rows(output, 'pick')
    assert len(got) == 12
    for word, n, pick in got:
        assert int(pick) == (int(word, 16) * int(n)) >> 32 and 0 <= int(pick) < int(n)


def test_segment_and_point_equal_the_model(output, lanes):
    pts = [[float.fromhex(v) for v in r] for r in rows(output, 'point')]
    assert len(pts) == len(POINTS)
    for got, want, cum in zip(pts, POINTS, lanes.cum[0]):
        assert all(same(g, w) for g, w in zip(got, want + (cum,))), (got, want, cum)
    cum = lanes.cum[0]
    assert cum[1] == cum[2] and cum[0] < cum[1] < cum[3] < cum[4]              # one segment without length
    arcs = rows(output, 'arc')
    want_arcs = [-1.5, 0.0, 2.5, cum[3], cum[1], cum[4], cum[4] + 1.0, math.nan, cum[1]]
    want_k = [0, 0, 0, 3, 2, 3, 3, 0, 1]                                        # the last row names the segment without length itself
    assert len(arcs) == len(want_arcs)
    c = lanes.cl[0]
    for i, (row, s, k) in enumerate(zip(arcs, want_arcs, want_k)):
        got_s, got_k = float.fromhex(row[0]), int(row[1])
        x, y, dx, dy, t = (float.fromhex(v) for v in row[2:])
        assert same(got_s, s) and got_k == k, (row, s, k)
        if i < len(arcs) - 1:
            assert lanes.segment_of(0, s) == k
        # Lanes.pose, in float64 and then as the step kernel rounds it
        mdx, mdy, mdz = float(c[k + 1][0] - c[k][0]), float(c[k + 1][1] - c[k][1]), float(c[k + 1][2] - c[k][2])
        seg = math.sqrt((mdx * mdx + mdy * mdy) + mdz * mdz)
        u = (s - cum[k]) / seg if seg > 0.0 else 0.0
        assert same(dx, mdx) and same(dy, mdy) and same(t, u), (row, mdx, mdy, u)
        assert same(x, float(c[k][0]) + u * mdx) and same(y, float(c[k][1]) + u * mdy), row
        if i < len(arcs) - 1 and not math.isnan(s):
            px, py, _, psin, pcos = lanes.pose(0, s)
            l2 = math.sqrt(dx * dx + dy * dy)
            assert l2 > 0.0
            assert [bits32(x), bits32(y), bits32(dy / l2), bits32(dx / l2)] == [bits32(px), bits32(py), bits32(psin), bits32(pcos)], (row, px, py)
    # the cases that make the signs matter are really in there
    assert math.copysign(1.0, float.fromhex(arcs[1][2])) == -1.0 and float.fromhex(arcs[1][2]) == 0.0        # x = -0 at the start
    assert float.fromhex(arcs[0][6]) < 0.0 and float.fromhex(arcs[6][6]) > 1.0                                 # extrapolated at both ends
    assert float.fromhex(arcs[8][6]) == 0.0 and float.fromhex(arcs[8][4]) == 0.0                               # no length: t = 0, not 0 / 0


def test_clean_under_the_sanitizers(output):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    # the runtimes are linked statically: the program does not depend on the order in which shared libraries are loaded
    program = build('lane_math_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    assert run(program) == output
