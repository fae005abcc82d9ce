"""
CPU model of lane-following NPC traffic (csrc/lanes.hip `tds_lane_snap`, csrc/follow.hip `tds_lane_follow_step`), numpy /
Python float64, brute force: no grid, no culling, one NPC and one point at a time.  Every expression is written in the order
include/tdship.h states and the kernels use, one IEEE rounding per operation, so that kernel and model can be compared bit for bit.
  (a) the lane graph from shared bound end points (its own, quadratic restatement of `lanelet2.lane_successors`);
  (b) the route stream: Philox4x32-10 keyed by the seed with two words folded in, counted by (scene id, NPC, hop);
  (c) snap: a pose onto the lanelet within tolerance whose direction its heading agrees with best;
  (d) the step: path, leader, IDM, integration, pose.
"""
import math

import numpy as np

F32 = np.float32
MASK = 0xFFFFFFFF
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KEY_FOLD = (0x4C414E45, 0x464F4C57)          # "LANE", "FOLW": what separates the route stream from spawn's for the same seed
MAX_HOPS, MAX_PIECES = 8, 256
IDM = (1.5, 2.0, 1.5, 2.0, 6.0)               # T, s0, a, b, b_max


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints) -> 4 words (Salmon et al., SC'11)"""
    c0, c1, c2, c3 = [int(c) & MASK for c in counter]
    k0, k1 = [int(k) & MASK for k in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def route_word(seed, scene_id, npc, hop):
    seed, scene_id = int(seed) & 0xFFFFFFFFFFFFFFFF, int(scene_id) & 0xFFFFFFFFFFFFFFFF
    key = ((seed & MASK) ^ KEY_FOLD[0], (seed >> 32) ^ KEY_FOLD[1])
    return philox4x32_10((scene_id & MASK, scene_id >> 32, int(npc) & MASK, int(hop) & MASK), key)[0]


def successors(lanelet_map):
    """list of lists: j follows i iff i's last left / right bound point ids are j's first ones; j != i; ascending"""
    ls = lanelet_map.laneletLayer
    out = []
    for i, a in enumerate(ls):
        row = []
        if len(a.left_ids) and len(a.right_ids):
            for j, b in enumerate(ls):
                if j != i and len(b.left_ids) and len(b.right_ids) and int(a.left_ids[-1]) == int(b.left_ids[0]) and \
                        int(a.right_ids[-1]) == int(b.right_ids[0]):
                    row.append(j)
        out.append(row)
    return out


class Lanes:
    """A lanelet map as the model reads it: per lanelet the outline ring, the centre line, its cumulative 3-D length (summed front to back
    as tds_lanes_create does), the excluded-tag flag and the successors."""

    def __init__(self, lanelet_map, tags_to_exclude=('parking',)):
        self.poly, self.cl, self.cum, self.flag, self.succ, self.seg = [], [], [], [], successors(lanelet_map), []
        for l in lanelet_map.laneletLayer:
            c = np.asarray(l.centerline, np.float64).reshape(-1, 3)
            cum = [0.0]
            for i in range(1, len(c)):
                dx, dy, dz = float(c[i][0] - c[i - 1][0]), float(c[i][1] - c[i - 1][1]), float(c[i][2] - c[i - 1][2])
                seg = math.sqrt((dx * dx + dy * dy) + dz * dz)
                cum.append(seg if i == 1 else cum[-1] + seg)
            self.poly.append(np.asarray(l.polygon2d(), np.float64))
            self.cl.append(c), self.cum.append(cum)
            self.flag.append(any(t in l.attributes for t in tags_to_exclude))
            # per segment: start point, unit vector, 2-D length (element by element: one rounding per operation, as in a loop)
            d = c[1:, :2] - c[:-1, :2]
            l2 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            with np.errstate(invalid='ignore', divide='ignore'):
                t = np.where(l2[:, None] > 0.0, d / l2[:, None], 0.0)
            self.seg.append(np.concatenate([c[:-1, :2], t, l2[:, None]], 1).reshape(-1, 5))

    def __len__(self):
        return len(self.cl)

    def eligible(self, l):
        return len(self.cl[l]) >= 2 and self.cum[l][-1] > 0.0 and math.isfinite(self.cum[l][-1])

    def length(self, l):
        return self.cum[l][-1]

    def segment_of(self, l, s):
        """clip(searchsorted(cum, s, 'right') - 1, 0, n - 2)"""
        cum = self.cum[l]
        k = 0
        while k < len(cum) and cum[k] <= s:
            k += 1
        return min(max(k - 1, 0), len(cum) - 2)

    def pose(self, l, s):
        """(x, y, psi, sin, cos) at arc length s, float32 each, as the step kernel writes them"""
        k = self.segment_of(l, s)
        c = self.cl[l]
        dx, dy, dz = float(c[k + 1][0] - c[k][0]), float(c[k + 1][1] - c[k][1]), float(c[k + 1][2] - c[k][2])
        seg = math.sqrt((dx * dx + dy * dy) + dz * dz)
        u = (s - self.cum[l][k]) / seg if seg > 0.0 else 0.0
        l2 = math.sqrt(dx * dx + dy * dy)
        x, y = F32(float(c[k][0]) + u * dx), F32(float(c[k][1]) + u * dy)
        if l2 > 0.0:
            return x, y, F32(math.atan2(dy, dx)), F32(dy / l2), F32(dx / l2)
        return x, y, F32(0), F32(0), F32(1)

    def successor(self, l, seed, scene_id, npc, hop):
        """the lanelet taken from `l` at hop `hop`; -1 at a dead end (no successor, or one nothing can drive on)"""
        s = self.succ[l]
        if not s:
            return -1
        j = s[(route_word(seed, scene_id, npc, hop) * len(s)) >> 32] if len(s) > 1 else s[0]
        return j if self.eligible(j) else -1


# ------------------------------------------------------------------------------------------------------------------------
# snap
# ------------------------------------------------------------------------------------------------------------------------
def ring_distance(poly, x, y):
    """distance from a point to the closed ring, 0 inside (even-odd rule), as boost::geometry::distance(point, polygon)"""
    n = len(poly)
    inside, best = False, math.inf
    for i in range(n):
        ax, ay = (float(v) for v in poly[i - 1])
        bx, by = (float(v) for v in poly[i])
        if (ay > y) != (by > y) and x < ax + (y - ay) * (bx - ax) / (by - ay):
            inside = not inside
        dx, dy = bx - ax, by - ay
        l2 = dx * dx + dy * dy
        t = ((x - ax) * dx + (y - ay) * dy) / l2 if l2 > 0 else 0.0
        t = min(max(t, 0.0), 1.0)
        fx, fy = ax + t * dx - x, ay + t * dy - y
        best = min(best, fx * fx + fy * fy)
    return 0.0 if inside else math.sqrt(best)


def foot(c, x, y):
    """closest point of the 2-D poly-line: (segment, u, unit tx, unit ty); the earliest segment on ties"""
    best, k = math.inf, -1
    for i in range(len(c) - 1):
        ax, ay = float(c[i][0]), float(c[i][1])
        dx, dy = float(c[i + 1][0]) - ax, float(c[i + 1][1]) - ay
        l2 = dx * dx + dy * dy
        u = ((x - ax) * dx + (y - ay) * dy) / l2 if l2 > 0 else 0.0
        u = min(max(u, 0.0), 1.0)
        fx, fy = ax + u * dx - x, ay + u * dy - y
        d2 = fx * fx + fy * fy
        if d2 < best:
            best, k = d2, i
    ax, ay = float(c[k][0]), float(c[k][1])
    dx, dy = float(c[k + 1][0]) - ax, float(c[k + 1][1]) - ay
    l2 = dx * dx + dy * dy
    u = ((x - ax) * dx + (y - ay) * dy) / l2 if l2 > 0 else 0.0
    u = min(max(u, 0.0), 1.0)
    ln = math.sqrt(l2)
    return k, u, (dx / ln if ln > 0 else 0.0), (dy / ln if ln > 0 else 0.0)


def snap(lanes, x, y, sn, cs, tolerance=1.0, with_scores=False):
    """x, y, sin, cos: float32 values (widened here).  -> (lane, arc float64, lateral float32); lane -1 when no candidate has a score > 0.
    with_scores: also the list of (lanelet, score, ring distance) of all candidates, for tests that keep away from the thresholds."""
    x, y, sn, cs = float(x), float(y), float(sn), float(cs)
    best = (-1, 0.0, 0.0)
    best_score, scores = 0.0, []
    for l in range(len(lanes)):
        if lanes.flag[l] or not lanes.eligible(l):
            continue
        d = ring_distance(lanes.poly[l], x, y)
        if not d <= tolerance:
            if with_scores and d <= tolerance + 0.01:
                scores.append((l, None, d))
            continue
        c = lanes.cl[l]
        k, u, tx, ty = foot(c, x, y)
        score = cs * tx + sn * ty
        scores.append((l, score, d))
        if score > best_score:
            cum = lanes.cum[l]
            best_score = score
            best = (l, cum[k] + u * (cum[k + 1] - cum[k]), tx * (y - float(c[k][1])) - ty * (x - float(c[k][0])))
    out = (best[0], best[1], F32(best[2]))
    return out + (scores,) if with_scores else out


# ------------------------------------------------------------------------------------------------------------------------
# the step
# ------------------------------------------------------------------------------------------------------------------------
def build_path(lanes, lane, arc, hops, seed, scene_id, npc, horizon):
    """-> (pieces (n, 6) [sx, sy, tx, ty, l2, off], smin, total, dead_end, lanelets visited).  The running path distance is summed front to
    back (np.cumsum adds in sequence), the first piece counting from where the NPC stands on it."""
    parts, off, smin, dead, n = [], 0.0, 0.0, False, 0
    l, hop, chain = lane, hops, [lane]
    for visited in range(MAX_HOPS + 1):
        c, seg = lanes.cl[l], lanes.seg[l]
        k0 = lanes.segment_of(l, arc) if visited == 0 else 0
        if visited == 0:
            dx, dy, dz = float(c[k0 + 1][0] - c[k0][0]), float(c[k0 + 1][1] - c[k0][1]), float(c[k0 + 1][2] - c[k0][2])
            s3 = math.sqrt((dx * dx + dy * dy) + dz * dz)
            u0 = (arc - lanes.cum[l][k0]) / s3 if s3 > 0.0 else 0.0
            smin = u0 * math.sqrt(dx * dx + dy * dy)
        avail = len(seg) - k0
        take = min(avail, MAX_PIECES - n)
        w = seg[k0:k0 + take, 4].copy()
        if visited == 0 and take > 0:
            w[0] = w[0] - smin
        run = np.cumsum(np.concatenate([[off], w]))                      # run[i] = path distance at the start of piece i of this lanelet
        reached = np.nonzero(run[1:] >= horizon)[0]
        used = int(reached[0]) + 1 if len(reached) else take
        parts.append(np.concatenate([seg[k0:k0 + used], run[:used, None]], 1))
        n, off = n + used, float(run[used])
        if len(reached) or take < avail or visited == MAX_HOPS:
            break
        nxt = lanes.successor(l, seed, scene_id, npc, hop)
        if nxt < 0:
            dead = True
            break
        l, hop = nxt, hop + 1
        chain.append(l)
    return np.concatenate(parts, 0), smin, off, dead, chain


def entity_points(boxes, sc):
    """(E, 5) boxes, (E, 2) [sin, cos], float32 -> (E, 5, 2) float64: the centre, then the corners (+,+), (+,-), (-,-), (-,+) of the box frame"""
    b, q = np.asarray(boxes, F32).astype(np.float64), np.asarray(sc, F32).astype(np.float64)
    ex, ey, hl, hw, es, ec = b[:, 0], b[:, 1], b[:, 2] / 2.0, b[:, 3] / 2.0, q[:, 0], q[:, 1]
    pts = [np.stack([ex, ey], -1)]
    for fl, fw in ((hl, hw), (hl, -hw), (-hl, -hw), (-hl, hw)):
        pts.append(np.stack([ex + (fl * ec - fw * es), ey + (fl * es + fw * ec)], -1))
    return np.stack(pts, 1)


def project(pieces, smin, px, py):
    """one point, piece by piece -> (path distance d, squared distance from the path, piece) of the closest point of the path, the earliest
    piece on ties; None for an empty path.  (`project_all` is the same for many points at once; the tests hold the two together.)"""
    best, bs, bi = math.inf, 0.0, -1
    for i, (sx, sy, tx, ty, l2, _) in enumerate(np.asarray(pieces).tolist()):
        s = (px - sx) * tx + (py - sy) * ty
        s = min(max(s, smin if i == 0 else 0.0), l2)
        fx, fy = px - (sx + s * tx), py - (sy + s * ty)
        d2 = fx * fx + fy * fy
        if d2 < best:
            best, bs, bi = d2, s, i
    if bi < 0:
        return None
    return float(pieces[bi][5]) + (bs - smin if bi == 0 else bs), best, bi


def project_all(pieces, smin, px, py):
    """(P,) points -> (d (P,), squared distance (P,), piece (P,)); element by element the arithmetic of `project`"""
    sx, sy, tx, ty, l2, off = (pieces[:, k] for k in range(6))
    lo = np.zeros(len(pieces))
    lo[0] = smin
    s = (px[:, None] - sx) * tx + (py[:, None] - sy) * ty
    s = np.minimum(np.maximum(s, lo), l2)
    fx, fy = px[:, None] - (sx + s * tx), py[:, None] - (sy + s * ty)
    d2 = fx * fx + fy * fy
    bi = d2.argmin(1)                                                      # the first of equal minima
    rows = np.arange(len(px))
    bs = s[rows, bi]
    return off[bi] + np.where(bi == 0, bs - smin, bs), d2[rows, bi], bi


def find_leader(pieces, smin, total, dead, boxes, sc, speed, present, self_index, own_len, own_wid, margin):
    """-> (leader, gap, v_lead); leader -1: none (gap, v_lead unused), -2: the end of the lane"""
    reach = own_wid / 2.0 + margin
    reach2 = reach * reach
    leader, gap, v_lead = -1, 0.0, 0.0
    E = len(boxes)
    if E > 0 and len(pieces) > 0:
        pts = entity_points(boxes, sc).reshape(-1, 2)                      # point p = 5 j + c
        d, d2, bi = project_all(pieces, smin, pts[:, 0], pts[:, 1])
        owner = np.repeat(np.arange(E), 5)
        ok = (d2 <= reach2) & (d > 0.0) & (owner != self_index) & np.repeat(np.asarray(present, bool), 5)
        if ok.any():
            p = int(np.where(ok, d, np.inf).argmin())                     # the smallest d, the lowest point index on ties
            j, i = int(owner[p]), int(bi[p])
            cos = float(sc[j][1]) * float(pieces[i][2]) + float(sc[j][0]) * float(pieces[i][3])
            leader, gap, v_lead = j, float(d[p]) - own_len / 2.0, float(speed[j]) * max(0.0, cos)
    if dead:
        end_gap = total - own_len / 2.0
        if leader == -1 or end_gap < gap:
            leader, gap, v_lead = -2, end_gap, 0.0
    return leader, gap, v_lead


def idm_acceleration(v, v0, leader, gap, v_lead, idm=IDM):
    T, s0, a, b, b_max = (float(F32(p)) for p in idm)
    r1 = v / v0
    r2 = r1 * r1
    acc = 1.0 - r2 * r2
    if leader != -1:
        gap = max(gap, 0.1)
        s_star = s0 + max(0.0, v * T + v * (v - v_lead) / (2.0 * math.sqrt(a * b)))
        q = s_star / gap
        acc = acc - q * q
    return max(-b_max, a * acc)


def step_npc(lanes, lane, arc, hops, speed, size, v0, boxes, sc, ent_speed, present, self_index, seed, scene_id, npc, dt, horizon=60.0,
             margin=0.2, idm=IDM):
    """One NPC, one step.  lane, hops: ints; arc: float64; speed, v0, size, boxes, sc, ent_speed: float32 values.
    -> dict(lane, arc, hops, speed (float32), x, y, psi, sin, cos (float32), leader, ds)"""
    dt, horizon, margin = float(F32(dt)), float(F32(horizon)), float(F32(margin))
    v, own_len, own_wid = float(speed), float(size[0]), float(size[1])
    pieces, smin, total, dead, _ = build_path(lanes, lane, arc, hops, seed, scene_id, npc, horizon)
    leader, gap, v_lead = find_leader(pieces, smin, total, dead, boxes, sc, ent_speed, present, self_index, own_len, own_wid, margin)
    acc = idm_acceleration(v, float(v0), leader, gap, v_lead, idm)
    v_new = F32(max(0.0, v + acc * dt))
    ds = (v + float(v_new)) / 2.0 * dt
    arc = arc + ds
    for _ in range(MAX_HOPS):
        length = lanes.length(lane)
        if not arc >= length:
            break
        nxt = lanes.successor(lane, seed, scene_id, npc, hops)
        if nxt < 0:
            arc, v_new = length, F32(0)
            break
        arc, lane, hops = arc - length, nxt, hops + 1
    if not arc <= lanes.length(lane):
        arc = lanes.length(lane)
    x, y, psi, sn, cs = lanes.pose(lane, arc)
    return dict(lane=lane, arc=arc, hops=hops, speed=v_new, x=x, y=y, psi=psi, sin=sn, cos=cs, leader=leader, ds=ds)


def step_scene(lanes, lane, arc, hops, state, size, v0, npc_present, boxes, sc, ent_speed, present, self_index, seed, scene_id, dt,
               horizon=60.0, margin=0.2, idm=IDM):
    """All NPCs of one scene (a Jacobi update: every NPC reads `boxes` as given).  Arrays per NPC in, a dict of arrays out; rows with lane < 0,
    not present or without a desired speed > 0 come back unchanged with leader -1 (their sin / cos are reported as NaN: the kernel leaves them as they were)."""
    N = len(lane)
    out = dict(lane=np.array(lane, np.int32), arc=np.array(arc, np.float64), hops=np.array(hops, np.int32), state=np.array(state, F32),
               sc=np.full((N, 2), np.nan, F32), leader=np.full(N, -1, np.int32), moved=np.zeros(N, bool))
    for n in range(N):
        if lane[n] < 0 or not npc_present[n] or not v0[n] > 0:
            continue
        r = step_npc(lanes, int(lane[n]), float(arc[n]), int(hops[n]), state[n][3], size[n], v0[n], boxes, sc, ent_speed, present,
                     int(self_index[n]), seed, scene_id, n, dt, horizon, margin, idm)
        out['lane'][n], out['arc'][n], out['hops'][n], out['leader'][n], out['moved'][n] = r['lane'], r['arc'], r['hops'], r['leader'], True
        out['state'][n] = (r['x'], r['y'], r['psi'], r['speed'])
        out['sc'][n] = (r['sin'], r['cos'])
    return out
