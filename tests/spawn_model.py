"""
CPU model of the on-lane spawn kernel (csrc/spawn.hip, `tds_spawn_on_lanes_f32`), numpy only:
  (a) Philox4x32-10;
  (b) the sampler: (seed, scene id, agent, attempt) -> eligible lanelet, arc length, speed -> point, heading, unit-vector [sin, cos] on a
      `lanelet2.LaneTable`, every step an exact IEEE expression (include/tdship.h states them);
  (c) the sequential accept loop of the reference's heuristic_initialize (behavior/heuristic.py:19-48), taking its decisions from
      `oracle.discs_pairs` -- the restatement pinned to the reference's recorded disc values (G2, G13).
The loop is one oracle call per attempt: slow on purpose, it is the definition the kernel is compared with.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
F32 = np.float32


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints) -> 4 words"""
    c0, c1, c2, c3 = [int(c) & MASK for c in counter]
    k0, k1 = [int(k) & MASK for k in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw(seed, scene_id, agent, attempt):
    seed, scene_id = int(seed) & 0xFFFFFFFFFFFFFFFF, int(scene_id) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((scene_id & MASK, scene_id >> 32, agent, attempt), (seed & MASK, seed >> 32))


class Lanes:
    """What tds_lanes_create keeps of a LaneTable for the sampler: per lanelet the centre line, its segment lengths, their running sum
    (float64, front to back) and the list of eligible lanelets (>= 2 points, finite positive length)."""

    def __init__(self, table):
        self.cl, self.seg, self.cum, self.eligible = [], [], [], []
        for l in range(len(table.flags)):
            c = np.asarray(table.cl_xyz[table.cl_start[l]:table.cl_start[l + 1]], np.float64)
            seg = np.sqrt(((c[1:] - c[:-1]) ** 2).sum(1)) if len(c) >= 2 else np.zeros(0)
            cum = np.concatenate([[0.0], np.cumsum(seg)])
            self.cl.append(c), self.seg.append(seg), self.cum.append(cum)
            if len(c) >= 2 and cum[-1] > 0 and np.isfinite(cum[-1]):
                self.eligible.append(l)

    def at(self, l, s):
        c, seg, cum = self.cl[l], self.seg[l], self.cum[l]
        k = int(np.clip(np.searchsorted(cum, s, side='right') - 1, 0, len(seg) - 1))
        t = (s - cum[k]) / seg[k] if seg[k] > 0 else 0.0
        return c[k] + t * (c[k + 1] - c[k])

    def length(self, l):
        return float(self.cum[l][-1])

    def point(self, l, s):
        """(x, y, psi) in float64 as lanelet2.pick_random_point_and_orientation returns them, and the unit vector [sin, cos] in float32"""
        p, q = self.at(l, s), self.at(l, min(s + 1, self.length(l)))
        dx, dy = float(q[0] - p[0]), float(q[1] - p[1])
        n = float(np.sqrt(np.float64(dx) * dx + np.float64(dy) * dy))
        if n > 0:
            return float(p[0]), float(p[1]), float(np.arctan2(dy, dx)), F32(dy / n), F32(dx / n)
        return float(p[0]), float(p[1]), 0.0, F32(0), F32(1)


def lane_and_distance(lanes, r):
    l = lanes.eligible[(r[0] * len(lanes.eligible)) >> 32]
    return l, lanes.length(l) * (float(r[1]) + 0.5) * 2.0 ** -32


def speed_of(r, min_speed, max_speed):
    lo, hi = F32(min_speed), F32(max_speed)
    return F32(lo + F32(F32(hi - lo) * F32(F32(r[2] >> 8) * F32(2.0 ** -24))))


def candidate(lanes, seed, scene_id, agent, attempt, min_speed=0, max_speed=10):
    """(x, y, psi, sin, cos, speed), float32 each, as the kernel forms them"""
    r = draw(seed, scene_id, agent, attempt)
    l, s = lane_and_distance(lanes, r)
    x, y, psi, sn, cs = lanes.point(l, s)
    return F32(x), F32(y), F32(psi), sn, cs, speed_of(r, min_speed, max_speed)


def metric_sc(sn, cs, length, width):
    """[sin, cos] of psi + pi/2 * (width > length), exactly: a quarter turn of the unit vector"""
    return (cs, F32(-sn)) if width > length else (sn, cs)


def accept_loop(orc, candidates, attributes, gap=(1.0, 0.2), max_attempts=500, occupied=None, occupied_sc=None):
    """The reference's loop over a candidate source.
    candidates(agent, attempt) -> (x, y, psi, sin, cos, speed); attributes (A, 3); occupied (M, 5) boxes NOT yet inflated with
    occupied_sc (M, 2) of the inflated boxes' metric angle.
    Returns states (A, 4), sc (A, 2), placed (A,) bool, attempts (A,) int32 -- zero rows from the first agent that finds no place."""
    A = len(attributes)
    states, sc = np.zeros((A, 4), F32), np.zeros((A, 2), F32)
    placed, attempts = np.zeros(A, bool), np.zeros(A, np.int32)
    gl, gw = F32(gap[0]), F32(gap[1])
    boxes, bsc = [], []
    if occupied is not None:
        for o, s in zip(np.asarray(occupied, F32), np.asarray(occupied_sc, F32)):
            boxes.append([o[0], o[1], F32(o[2] + gl), F32(o[3] + gw), o[4]])
            bsc.append([s[0], s[1]])
    for i in range(A):
        length, width = F32(attributes[i][0]), F32(attributes[i][1])
        for a in range(max_attempts):
            x, y, psi, sn, cs, v = candidates(i, a)
            attempts[i] = a + 1
            free = True
            if boxes:
                me = np.tile(np.array([x, y, length, width, psi], F32), (len(boxes), 1))
                msc = np.tile(np.array(metric_sc(sn, cs, length, width), F32), (len(boxes), 1))
                free = not bool((orc.discs_pairs(me, np.array(boxes, F32), msc, np.array(bsc, F32)) > 0).any())
            if free:
                states[i], sc[i], placed[i] = (x, y, psi, v), (sn, cs), True
                il, iw = F32(length + gl), F32(width + gw)
                boxes.append([x, y, il, iw, psi])
                bsc.append(list(metric_sc(sn, cs, il, iw)))
                break
        if not placed[i]:
            break
    return states, sc, placed, attempts


def spawn_scene(orc, lanes, seed, scene_id, attributes, min_speed=0, max_speed=10, max_attempts=500, gap=(1.0, 0.2), occupied=None,
                occupied_sc=None):
    """One scene of tds_spawn_on_lanes_f32.  A table without an eligible lanelet places nothing and draws nothing."""
    if not lanes.eligible:
        A = len(attributes)
        return np.zeros((A, 4), F32), np.zeros((A, 2), F32), np.zeros(A, bool), np.zeros(A, np.int32)
    return accept_loop(orc, lambda i, a: candidate(lanes, seed, scene_id, i, a, min_speed, max_speed), attributes, gap, max_attempts,
                       occupied, occupied_sc)


def default_attributes(n):
    return np.tile(np.array([4.97, 2.04, 1.96], F32), (n, 1))
