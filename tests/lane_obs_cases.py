"""
The small synthetic lane maps and observer poses the lane-observation tests share (tests/test_lane_obs_model.py on the CPU,
tests/test_gpu_lane_obs.py on the GPU): a chain of three lanelets, a fork, a dead end beside an oncoming lane, a loop of two lanelets, lanelets
with an excluded tag, a ring of 70 short lanelets.  Lanelets follow one another through shared bound END POINT IDS (`lanelet2.lane_successors`),
so the ids are given by hand: junction j has the ids (2 j + 1, 2 j + 2) for the left and the right bound.
"""
import math

import numpy as np

from torchdrivesim_amd import lanelet2

HALF = 1.5          # half a lane's width


def lanelet(ident, centre, j0, j1, tag=None, half=HALF):
    """a lanelet around the 2-D poly-line `centre`, from junction j0 to junction j1"""
    c = np.asarray(centre, np.float64)
    d = np.gradient(c, axis=0)
    nrm = np.stack([-d[:, 1], d[:, 0]], 1) / np.hypot(d[:, 0], d[:, 1])[:, None]
    z = np.zeros((len(c), 1))
    mid = 1000 * ident + np.arange(1, len(c) - 1)
    left_ids = np.concatenate([[2 * j0 + 1], 2 * mid, [2 * j1 + 1]])
    right_ids = np.concatenate([[2 * j0 + 2], 2 * mid + 1, [2 * j1 + 2]])
    return lanelet2.Lanelet(ident, np.concatenate([c + half * nrm, z], 1), np.concatenate([c - half * nrm, z], 1), left_ids, right_ids,
                            {'parking': 'yes'} if tag else {})


def make_map(lanelets):
    return lanelet2.LaneletMap([], np.zeros((0, 3)), lanelets)


def arc_points(cx, cy, radius, a0, a1, n):
    return [(cx + radius * math.cos(a), cy + radius * math.sin(a)) for a in np.linspace(a0, a1, n)]


def chain():
    """0 -> 1 -> 2 along +x, 10 m each; lanelet 1 has two segments; the end of 2 is a dead end"""
    return make_map([lanelet(0, [(0, 0), (10, 0)], 0, 1), lanelet(1, [(10, 0), (15, 0), (20, 0)], 1, 2), lanelet(2, [(20, 0), (30, 0)], 2, 3)])


def fork():
    """0 is followed by 1 (straight on) and 2 (bending left): two successors, the polyline of 0 ends at its end"""
    return make_map([lanelet(0, [(0, 0), (10, 0)], 0, 1), lanelet(1, [(10, 0), (20, 0)], 1, 2),
                     lanelet(2, [(10, 0), (13, 0.5), (16, 2), (19, 5)], 1, 3)])


def dead_end():
    """0 bends and ends; 1 is the oncoming lane beside it, connected to nothing"""
    return make_map([lanelet(0, [(0, 0), (5, 0), (12, 3)], 0, 1), lanelet(1, [(12, 7), (5, 4), (0, 4)], 2, 3)])


def loop():
    """0 -> 1 -> 0: two half circles of radius 4 (about 12.4 m each), so that 31 points 4 m apart run into the hop limit"""
    return make_map([lanelet(0, arc_points(0, 0, 4, 0, math.pi, 7), 0, 1), lanelet(1, arc_points(0, 0, 4, math.pi, 2 * math.pi, 7), 1, 0)])


def tagged():
    """0 -> 2, 2 carries an excluded tag (the polyline of 0 ends at its end); 1 lies beside 0 and is tagged too; 3 is a plain lane on the
    other side"""
    return make_map([lanelet(0, [(0, 0), (10, 0)], 0, 1), lanelet(1, [(0, 3), (10, 3)], 2, 3, tag=True), lanelet(2, [(10, 0), (20, 0)], 1, 4, tag=True),
                     lanelet(3, [(0, -3), (10, -3)], 5, 6)])


def ring(n=70, radius=40.0):
    """n short lanelets round a circle, each followed by the next: more than 64 lanelets, the form of the selection that keeps its keys in LDS"""
    out = []
    for i in range(n):
        a0, a1 = 2 * math.pi * i / n, 2 * math.pi * (i + 1) / n
        out.append(lanelet(i, arc_points(0, 0, radius, a0, a1, 3), i, (i + 1) % n))
    return make_map(out)


def edge():
    """one lanelet that ends 2^-23 m short of x = 10: from (10, 10) its end is at d2 = 100 + 2^-46, ONE binary64 step beyond 10 m"""
    return make_map([lanelet(0, [(0, 0), (10 - 2.0 ** -23, 0)], 0, 1)])


STRUCTURES = dict(edge=edge, chain=chain, fork=fork, dead_end=dead_end, loop=loop, tagged=tagged)


#: poses (x, y, psi) every synthetic map is also seen from: the definition's cases by hand (tests/test_lane_obs_model.py says what each one is)
HAND_POSES = [(5.0, 3.0, 0.0), (10.0, 3.0, 0.0), (2.0, 0.0, 0.0), (5.0, 50.0, 0.0), (math.nan, 0.0, 0.0), (0.0, math.nan, 0.0), (4.0, 0.0, math.pi / 2),
              (5.0, 10.0, 0.0), (5.0, float(np.nextafter(np.float32(10.0), np.float32(11.0))), 0.0), (10.0, 10.0, 0.0), (5.0, 0.0, math.nan),
              (2.0, 0.5, math.pi)]


def poses(rng, lanelet_map, n, spread=6.0):
    """n observer poses (x, y, psi) float32 around the centre lines of a map, the first few exactly ON centre-line points"""
    pts = np.concatenate([l.centerline[:, :2] for l in lanelet_map.laneletLayer], 0)
    pick = pts[rng.integers(0, len(pts), n)]
    xy = pick + rng.normal(0.0, spread, (n, 2))
    xy[:min(2, n)] = pick[:min(2, n)]
    return np.concatenate([xy, rng.uniform(-math.pi, math.pi, (n, 1))], 1).astype(np.float32)
