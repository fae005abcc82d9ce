"""
CPU model of giving way at junctions (csrc/conflicts.hip `tds_lane_conflicts_f64`, `tds_lane_give_way_multi`; csrc/follow.hip with `stop_at`;
DESIGN.md 5.5j), numpy / Python float64 on top of tests/lane_follow_model.py.  Every expression is written in the order include/tdship.h states
and csrc/tds_conflicts.h uses, one IEEE rounding per operation, so that kernels and model can be compared bit for bit.
  (a) the conflict table of a map: per ordered pair of lanelets the last sample of a's centre line within the clearance of b's;
  (b) the yield pass: per NPC the junction on its path, whether it is committed or held, and whom it gives way to;
  (c) the step of lane_follow_model with the stop of (b) as one more standing obstacle.
"""
import math

import numpy as np

import lane_follow_model as lf

F32 = np.float32
MAX_SAMPLES = 1 << 20                         # tds::CONFLICT_MAX_SAMPLES
MAX_LANELETS, MAX_NPCS = 2048, 1024           # TDS_CONFLICT_MAX_LANELETS, TDS_GIVE_WAY_MAX_NPCS
CLEARANCE, STEP, CREEP_SPEED = 2.0, 0.5, 1.0


# ------------------------------------------------------------------------------------------------------------------------
# (a) the conflict table
# ------------------------------------------------------------------------------------------------------------------------
def excluded(lanes):
    """per lanelet a the set of b that are the same stream: a itself, its successors, its predecessors, the other successors of a predecessor"""
    out = [{a} for a in range(len(lanes))]
    for p, succ in enumerate(lanes.succ):
        for s in succ:
            out[p].add(s), out[s].add(p)
            out[s].update(succ)
    return out


def sample_points(lanes, a, step):
    """(arcs (n,), x (n,), y (n,)) of the samples k = 0 .. floor(length / step) of lanelet a, each the point at its arc (tds::point_at_arc)"""
    q = math.floor(lanes.length(a) / step)
    last = min(int(q), MAX_SAMPLES)
    s = np.arange(last + 1, dtype=np.float64) * step
    cum, c = np.asarray(lanes.cum[a], np.float64), lanes.cl[a]
    k = np.clip(np.searchsorted(cum, s, side='right') - 1, 0, len(cum) - 2)
    dx, dy, dz = c[k + 1, 0] - c[k, 0], c[k + 1, 1] - c[k, 1], c[k + 1, 2] - c[k, 2]
    seg = np.sqrt((dx * dx + dy * dy) + dz * dz)
    with np.errstate(invalid='ignore', divide='ignore'):
        t = np.where(seg > 0.0, (s - cum[k]) / seg, 0.0)
    return s, c[k, 0] + t * dx, c[k, 1] + t * dy


def within_clearance(c, x, y, clearance2):
    """(n,) points against the 2-D segments of centre line c: the least squared distance (tds::segment_foot) <= clearance^2"""
    ax, ay = c[:-1, 0], c[:-1, 1]
    dx, dy = c[1:, 0] - ax, c[1:, 1] - ay
    l2 = dx * dx + dy * dy
    with np.errstate(invalid='ignore', divide='ignore'):
        u = np.where(l2 > 0, ((x[:, None] - ax) * dx + (y[:, None] - ay) * dy) / l2, 0.0)
    u = np.fmin(np.fmax(u, 0.0), 1.0)
    fx, fy = ax + u * dx - x[:, None], ay + u * dy - y[:, None]
    d2 = fx * fx + fy * fy
    return np.fmin.reduce(d2, axis=1, initial=np.inf) <= clearance2


def conflict_tables(lanes, clearance=CLEARANCE, step=STEP):
    """-> (exit (L, L), zone_in (L,), zone_out (L,)) float64.  Pairs whose centre lines' bounding boxes are further apart than the clearance are
    skipped: none of their samples can hit."""
    clearance, step = float(F32(clearance)), float(F32(step))
    L = len(lanes)
    exit_, zone_in, zone_out = np.full((L, L), -1.0), np.full(L, np.inf), np.full(L, -1.0)
    ok = [lanes.eligible(l) for l in range(L)]
    box = [(lanes.cl[l][:, :2].min(0), lanes.cl[l][:, :2].max(0)) if ok[l] else None for l in range(L)]
    same_stream = excluded(lanes)
    c2 = clearance * clearance
    for a in range(L):
        if not ok[a]:
            continue
        s, x, y = sample_points(lanes, a, step)
        for b in range(L):
            if not ok[b] or b in same_stream[a]:
                continue
            gap = np.maximum(box[a][0] - box[b][1], box[b][0] - box[a][1]).max()
            if gap > clearance + 1e-6:
                continue
            hit = np.nonzero(within_clearance(lanes.cl[b], x, y, c2))[0]
            if len(hit):
                exit_[a, b] = s[hit[-1]]
                zone_in[a], zone_out[a] = min(zone_in[a], s[hit[0]]), max(zone_out[a], s[hit[-1]])
    return exit_, zone_in, zone_out


def conflicting(tables):
    """(L, L) bool: exit[a][b] >= 0 and exit[b][a] >= 0"""
    return (tables[0] >= 0) & (tables[0].T >= 0)


# ------------------------------------------------------------------------------------------------------------------------
# (b) the yield pass
# ------------------------------------------------------------------------------------------------------------------------
def summary(lanes, tables, lane, arc, hops, v, length, seed, scene_id, npc, lines, horizon, b_max, creep_speed):
    """the junction on one NPC's path: None, or dict(junction, start, half, D, gap, t, committed, held).  lines: [(lanelet, arc, red)]"""
    _, zone_in, zone_out = tables
    half = length / 2.0
    l, start, seen = lane, -arc, []
    for k in range(lf.MAX_HOPS + 1):
        seen.append((l, start))
        zi, zo = float(zone_in[l]), float(zone_out[l])
        if zo >= 0.0 and start + zo + half > 0.0 and start + zi <= horizon:
            D = start + zi
            gap = D - half
            committed = gap <= 0.0 or v * v >= 2.0 * b_max * gap
            t = max(gap, 0.0) / max(v, creep_speed)
            held = not committed and any(red and ll == lk and 0.0 < sk + la and sk + la < start + zo for lk, sk in seen for ll, la, red in lines)
            return dict(junction=l, start=start, half=half, D=D, gap=gap, t=t, committed=committed, held=held)
        nxt_start = start + lanes.length(l)
        if nxt_start >= horizon or k == lf.MAX_HOPS:
            break
        nxt = lanes.successor(l, seed, scene_id, npc, hops + k)
        if nxt < 0:
            break
        l, start = nxt, nxt_start
    return None


def give_way(lanes, tables, lane, arc, hops, speed, size, present, seed, scene_id, lines=(), horizon=60.0, b_max=lf.IDM[4], creep_speed=CREEP_SPEED):
    """All NPCs of one scene as they are before the step -> (stop_at (N,) float64, yield_to (N,) int32, the summaries).  speed, size: float32."""
    horizon, b_max, creep_speed = float(F32(horizon)), float(F32(b_max)), float(F32(creep_speed))
    N = len(lane)
    stop_at, yield_to = np.full(N, np.inf), np.full(N, -1, np.int32)
    exit_ = None if tables is None else tables[0]
    s = [None] * N
    for i in range(N):
        if tables is not None and present[i] and 0 <= lane[i] < len(lanes) and lanes.eligible(int(lane[i])):
            s[i] = summary(lanes, tables, int(lane[i]), float(arc[i]), int(hops[i]), float(speed[i]), float(size[i][0]), seed, scene_id, i,
                           [(int(a), float(b), bool(c)) for a, b, c in lines], horizon, b_max, creep_speed)
    for i in range(N):
        if s[i] is None or s[i]['committed']:
            continue
        p = s[i]['junction']
        for j in range(N):
            if j == i or s[j] is None or s[j]['held']:
                continue
            q = s[j]['junction']
            if not (exit_[q, p] >= 0.0 and exit_[p, q] >= 0.0) or not s[j]['start'] + float(exit_[q, p]) + s[j]['half'] > 0.0:
                continue
            if s[j]['committed'] or s[j]['t'] < s[i]['t'] or (s[j]['t'] == s[i]['t'] and j < i):
                stop_at[i], yield_to[i] = s[i]['D'], j
                break
    return stop_at, yield_to, s


# ------------------------------------------------------------------------------------------------------------------------
# (c) the step
# ------------------------------------------------------------------------------------------------------------------------
def step_npc(lanes, lane, arc, hops, speed, size, v0, boxes, sc, ent_speed, present, self_index, seed, scene_id, npc, dt, stop_at, horizon=60.0,
             margin=0.2, idm=lf.IDM):
    """lane_follow_model.step_npc with one more obstacle: a finite stop_at, weighed after the leader and the dead end (leader -3)"""
    dt, horizon, margin = float(F32(dt)), float(F32(horizon)), float(F32(margin))
    v, own_len, own_wid = float(speed), float(size[0]), float(size[1])
    pieces, smin, total, dead, _ = lf.build_path(lanes, lane, arc, hops, seed, scene_id, npc, horizon)
    leader, gap, v_lead = lf.find_leader(pieces, smin, total, dead, boxes, sc, ent_speed, present, self_index, own_len, own_wid, margin)
    if math.isfinite(stop_at):
        gap_s = stop_at - own_len / 2.0
        if leader == -1 or gap_s < gap:
            leader, gap, v_lead = -3, gap_s, 0.0
    acc = lf.idm_acceleration(v, float(v0), leader, gap, v_lead, idm)
    v_new = F32(max(0.0, v + acc * dt))
    ds = (v + float(v_new)) / 2.0 * dt
    arc = arc + ds
    for _ in range(lf.MAX_HOPS):
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


def step_scene(lanes, tables, lane, arc, hops, state, size, v0, npc_present, boxes, sc, ent_speed, present, self_index, seed, scene_id, dt, lines=(),
               horizon=60.0, margin=0.2, idm=lf.IDM, creep_speed=CREEP_SPEED):
    """lane_follow_model.step_scene behind the yield pass; the dict also holds stop_at and yield_to"""
    N = len(lane)
    stop_at, yield_to, _ = give_way(lanes, tables, lane, arc, hops, np.asarray(state)[:, 3] if N else [], size, npc_present, seed, scene_id, lines, horizon,
                                    idm[4], creep_speed)
    out = dict(lane=np.array(lane, np.int32), arc=np.array(arc, np.float64), hops=np.array(hops, np.int32), state=np.array(state, F32),
               sc=np.full((N, 2), np.nan, F32), leader=np.full(N, -1, np.int32), moved=np.zeros(N, bool), stop_at=stop_at, yield_to=yield_to)
    for n in range(N):
        if lane[n] < 0 or not npc_present[n] or not v0[n] > 0:
            continue
        r = step_npc(lanes, int(lane[n]), float(arc[n]), int(hops[n]), state[n][3], size[n], v0[n], boxes, sc, ent_speed, present, int(self_index[n]),
                     seed, scene_id, n, dt, float(stop_at[n]), horizon, margin, idm)
        out['lane'][n], out['arc'][n], out['hops'][n], out['leader'][n], out['moved'][n] = r['lane'], r['arc'], r['hops'], r['leader'], True
        out['state'][n] = (r['x'], r['y'], r['psi'], r['speed'])
        out['sc'][n] = (r['sin'], r['cos'])
    return out
