"""
CPU model of the lane observations (K8: csrc/lane_obs.hip `tds_lane_observations_multi`, `Simulator.compute_lanes`; include/tdship.h "K8",
DESIGN.md 5.5i), numpy / Python float64, brute force: every lanelet, every segment, no box test, no LDS.  Every expression is written in the order
include/tdship.h states and the kernel uses, one IEEE rounding per operation (numpy's element-wise float64 operations and Python's floats round
once each), so that kernel and model can be compared bit for bit.  The lane table is `lane_follow_model.Lanes`: the centre lines, their
cumulative 3-D lengths summed as tds_lanes_create sums them, the excluded-tag flags and the successors.
"""
import math

import numpy as np

from lane_follow_model import Lanes  # noqa: F401  (what callers build the table with)

F32 = np.float32
MAX_HOPS, MAX_K, MAX_POINTS, MAX_LANELETS = 8, 32, 32, 2048
FEATURES = 8


def usable(lanes, l):
    """a candidate lanelet: drivable (>= 2 centre-line points, a finite positive length) and without an excluded tag"""
    return 0 <= l < len(lanes) and not lanes.flag[l] and lanes.eligible(l)


def segment_foot(c, i, x, y):
    """segment i of the centre line c against the pose (x, y), plain Python floats -> (ax, ay, dx, dy, l2, u, fx, fy, d2): tds::segment_foot"""
    ax, ay = float(c[i][0]), float(c[i][1])
    dx, dy = float(c[i + 1][0]) - ax, float(c[i + 1][1]) - ay
    l2 = dx * dx + dy * dy
    u = ((x - ax) * dx + (y - ay) * dy) / l2 if l2 > 0 else 0.0
    u = 0.0 if u != u else min(max(u, 0.0), 1.0)                     # fmin(fmax(u, 0), 1): a NaN gives 0
    fx, fy = ax + u * dx - x, ay + u * dy - y
    return ax, ay, dx, dy, l2, u, fx, fy, fx * fx + fy * fy


def feet(lanes, x, y):
    """The foot of the pose on every lanelet's 2-D centre line -> (d2 (L,) float64, sb (L,) int): the smallest d2 and the earliest segment that
    has it; sb = -1 where the lanelet is no candidate (not usable, or no d2 below +inf).  All segments of a lanelet at once, element by element
    the arithmetic of `segment_foot` (tests/test_lane_obs_model.py holds the two together)."""
    x, y = float(x), float(y)
    L = len(lanes)
    best, sb = np.full(L, np.inf), np.full(L, -1, np.int64)
    for l in range(L):
        if not usable(lanes, l):
            continue
        c = lanes.cl[l]
        ax, ay = c[:-1, 0], c[:-1, 1]
        dx, dy = c[1:, 0] - ax, c[1:, 1] - ay
        l2 = dx * dx + dy * dy
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            u = np.where(l2 > 0, ((x - ax) * dx + (y - ay) * dy) / l2, 0.0)
            u = np.fmin(np.fmax(u, 0.0), 1.0)
            fx, fy = ax + u * dx - x, ay + u * dy - y
            d2 = fx * fx + fy * fy
        ok = d2 < np.inf                                             # a NaN fails
        if ok.any():
            i = int(np.where(ok, d2, np.inf).argmin())               # the first of equal minima
            best[l], sb[l] = d2[i], i
    return best, sb


def select(d2, sb, k, max_distance):
    """the lanelets of the k slots, nearest first: the candidates with d2 <= r2 by (bits of float32(d2), l)"""
    md = float(F32(max_distance))
    r2 = md * md
    with np.errstate(over='ignore'):
        keys = [(int(F32(d2[l]).view(np.uint32)), l) for l in range(len(d2)) if sb[l] >= 0 and d2[l] <= r2]
    return [l for _, l in sorted(keys)[:k]]


def walk(lanes, l, q):
    """the lanelet and the arc length on it that q metres from the start of l lead to over unique successors, None for an invalid point"""
    cur, base, hops = l, 0.0, 0
    while q - base > lanes.length(cur):
        succ = lanes.succ[cur]
        if len(succ) != 1 or not usable(lanes, succ[0]) or hops >= MAX_HOPS:
            return None
        base, cur, hops = base + lanes.length(cur), succ[0], hops + 1
    return cur, q - base


def point_at(lanes, l, pos):
    """the world point at arc length pos of lanelet l, measured on `cum` (the convention of the route points) -> (wx, wy, segment, t)"""
    c, cum = lanes.cl[l], lanes.cum[l]
    k = lanes.segment_of(l, pos)
    w = cum[k + 1] - cum[k]
    t = (pos - cum[k]) / w if w > 0.0 else 0.0
    wx = float(c[k][0]) + t * (float(c[k + 1][0]) - float(c[k][0]))
    wy = float(c[k][1]) + t * (float(c[k + 1][1]) - float(c[k][1]))
    return wx, wy, k, t


def observe(lanes, pose, present, k, n_points, spacing, max_distance, found=None):
    """One observer.  pose: (x, y, sin, cos) float32 values; lanes: a `Lanes` or None (a scene without a map); found: `feet` of this pose when the
    caller has it already.  -> features (k, 8) float32, points (k, n_points, 2) float32, n_valid (k,) int32, index (k,) int32"""
    features, points = np.zeros((k, FEATURES), F32), np.zeros((k, n_points, 2), F32)
    n_valid, index = np.zeros(k, np.int32), np.full(k, -1, np.int32)
    x, y, s, c = (float(F32(v)) for v in pose)
    if not present or lanes is None or any(v != v for v in (x, y, s, c)):
        return features, points, n_valid, index
    d2, sb = feet(lanes, x, y) if found is None else found
    spacing = float(F32(spacing))
    with np.errstate(over='ignore'):
        for slot, l in enumerate(select(d2, sb, k, max_distance)):
            cl, cum = lanes.cl[l], lanes.cum[l]
            i = int(sb[l])
            ax, ay, dx, dy, l2, u, fx, fy, dd = segment_foot(cl, i, x, y)
            ln = math.sqrt(l2)
            tx, ty = (dx / ln, dy / ln) if ln > 0 else (0.0, 0.0)
            arc = cum[i] + u * (cum[i + 1] - cum[i])
            features[slot] = [F32(fx * c + fy * s), F32(fy * c - fx * s), F32(ty * c - tx * s), F32(tx * c + ty * s), F32(arc), F32(cum[-1] - arc),
                              F32(tx * (y - ay) - ty * (x - ax)), F32(math.sqrt(dd))]
            index[slot] = l
            for j in range(n_points):
                at = walk(lanes, l, arc + float(j) * spacing)
                if at is None:
                    break
                wx, wy, _, _ = point_at(lanes, *at)
                ex, ey = wx - x, wy - y
                points[slot, j] = [F32(ex * c + ey * s), F32(ey * c - ex * s)]
                n_valid[slot] = j + 1
    return features, points, n_valid, index


def observe_batch(scene_lanes, xy, sc, present, k, n_points, spacing, max_distance, found=None):
    """scene_lanes: per scene a `Lanes` or None; xy, sc (B, A, 2) float32, present (B, A); found: None or a dict (b, a) -> `feet` to reuse and
    fill.  -> features (B, A, k, 8), points (B, A, k, n_points, 2), n_valid (B, A, k), index (B, A, k)"""
    B, A = np.asarray(xy).shape[:2]
    out = (np.zeros((B, A, k, FEATURES), F32), np.zeros((B, A, k, n_points, 2), F32), np.zeros((B, A, k), np.int32), np.zeros((B, A, k), np.int32))
    for b in range(B):
        for a in range(A):
            lanes = scene_lanes[b]
            pose = (xy[b][a][0], xy[b][a][1], sc[b][a][0], sc[b][a][1])
            got = None
            if found is not None and lanes is not None and present[b][a] and not any(float(v) != float(v) for v in pose):
                if (b, a) not in found:
                    found[(b, a)] = feet(lanes, float(F32(pose[0])), float(F32(pose[1])))
                got = found[(b, a)]
            for o, r in zip(out, observe(lanes, pose, present[b][a], k, n_points, spacing, max_distance, got)):
                o[b, a] = r
    return out
