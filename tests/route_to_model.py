"""
CPU model of routes to a destination (csrc/route_to.hip; DESIGN.md 5.5e, include/tdship.h), Python float64, brute force.  Every expression is
written in the order the header states and the kernels use, one IEEE rounding per operation, so that kernel and model can be compared bit for bit.
  (a) distance_table: to_go[t][l], the distance from the START of lanelet l to the START of lanelet t, as plain sweeps to the fixed point;
  (b) dijkstra: the same table from a heap Dijkstra on the reversed graph -- an independent second opinion, not what the kernel does;
  (c) deal: the shortest route from (lane, arc) to (dest_lane, dest_arc), at most 16 lanelets, and `rest`, what is left after them.
The table does not depend on the order of relaxation: it is the least fixed point of d -> len + min d, and rounded addition is monotone.
"""
import heapq
import math

import numpy as np

from route_model import MAX_LANES, Lanes, Route, ring_with_fork  # noqa: F401  (Lanes, ring_with_fork: what the tests build the maps with)

MAX_GRAPH = 2048                              # TDS_ROUTE_MAX_GRAPH


def usable(lanes, l):
    """a lanelet a route may use: one that can be driven on and carries no excluded tag"""
    return 0 <= l < len(lanes) and lanes.eligible(l) and not lanes.flag[l]


def distance_table(lanes):
    """(L, L) float64, row t = the field of destination t; Jacobi sweeps until nothing changes, at most L of them"""
    L = len(lanes)
    table = np.full((L, L), math.inf)
    for t in range(L):
        d = [math.inf] * L
        if usable(lanes, t):
            d[t] = 0.0
        for _ in range(L):
            new, changed = list(d), False
            for l in range(L):
                if l == t or not usable(lanes, l):
                    continue
                m = math.inf
                for s in lanes.succ[l]:
                    if usable(lanes, s) and d[s] < m:
                        m = d[s]
                v = lanes.length(l) + m
                if v < d[l]:
                    new[l], changed = v, True
            d = new
            if not changed:
                break
        table[t] = d
    return table


def dijkstra(lanes):
    """the same table: per destination a heap Dijkstra over the predecessors"""
    L = len(lanes)
    pred = [[] for _ in range(L)]
    for l in range(L):
        for s in lanes.succ[l]:
            pred[s].append(l)
    table = np.full((L, L), math.inf)
    for t in range(L):
        if not usable(lanes, t):
            continue
        d = table[t]
        d[t] = 0.0
        heap, done = [(0.0, t)], set()
        while heap:
            du, u = heapq.heappop(heap)
            if u in done:
                continue
            done.add(u)
            for p in pred[u]:
                if p == t or not usable(lanes, p):
                    continue
                nd = lanes.length(p) + du
                if nd < d[p]:
                    d[p] = nd
                    heapq.heappush(heap, (nd, p))
    return table


def deal(lanes, table, lane, arc, dest_lane, dest_arc, present=True):
    """-> (Route, rest).  No route: (Route() with n = 0, inf); a route of zero length: (Route(), 0.0)"""
    l0, t = int(lane), int(dest_lane)
    if lanes is None or table is None or not present or not usable(lanes, l0) or not usable(lanes, t):
        return Route(), math.inf
    to_go = table[t]
    a, b = float(arc), float(dest_arc)
    if not a > 0.0:
        a = 0.0
    if a > lanes.length(l0):
        a = lanes.length(l0)
    if not b > 0.0:
        b = 0.0
    if b > lanes.length(t):
        b = lanes.length(t)
    a0, off, chain, offsets, bend, rest = a, 0.0, [], [], 0.0, math.inf
    if t == l0 and b >= a0:
        chain.append(l0), offsets.append(off)
        bend = b
        off = off + (bend - a)
        rest = 0.0
    else:
        l = l0
        for j in range(MAX_LANES):
            length = lanes.length(l)
            chain.append(l), offsets.append(off)
            bend = length
            off = off + (length - a)
            nxt, best = -1, math.inf
            for s in lanes.succ[l]:
                if usable(lanes, s) and float(to_go[s]) < best:
                    best, nxt = float(to_go[s]), s
            if nxt < 0:
                return Route(), math.inf
            if nxt == t and not b > 0.0:
                rest = 0.0
                break
            if j == MAX_LANES - 1:
                rest = best + b
                break
            if nxt == t:
                chain.append(t), offsets.append(off)
                bend = b
                off = off + (bend - 0.0)
                rest = 0.0
                break
            l, a = nxt, 0.0
    if not off > 0.0:
        return Route(), rest
    return Route(chain, a0, bend, offsets, off), rest


# ------------------------------------------------------------------------------------------------------------------------
# the second hand-built map of the tests
# ------------------------------------------------------------------------------------------------------------------------
def diamond(reach=5.0, bulge=3.0, half_width=1.0):
    """0 -> {1, 2} -> 3 -> 0: lanelet 0 runs along +x to a fork, legs 1 and 2 are mirror images of each other in the x axis and meet again at the
    start of lanelet 3, which goes round below and back to the start of lanelet 0.  Centre lines are set by hand; lanelets are joined through
    shared bound end point ids, as in a map file.  The legs' lengths are sums of the same numbers, so the fork is an EXACT tie."""
    from torchdrivesim_amd import lanelet2

    def lanelet(ident, centre, ids):
        c = np.asarray(centre, np.float64)
        d = np.gradient(c, axis=0)
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        normal = np.stack([-d[:, 1], d[:, 0]], 1) * half_width
        z = np.zeros((len(c), 1))
        mid = np.arange(1, len(c) - 1)
        left_ids = np.concatenate([[ids[0]], 1000 * ident + mid, [ids[2]]])
        right_ids = np.concatenate([[ids[1]], 2000 * ident + mid, [ids[3]]])
        return lanelet2.Lanelet(ident, np.concatenate([c + normal, z], 1), np.concatenate([c - normal, z], 1), left_ids, right_ids,
                                {'type': 'lanelet'}, np.concatenate([c, z], 1))

    r = reach
    out = [lanelet(1, [[0.0, 0.0], [r, 0.0], [2 * r, 0.0]], (300, 400, 301, 401)),
           lanelet(2, [[2 * r, 0.0], [3 * r, bulge], [4 * r, 0.0]], (301, 401, 302, 402)),
           lanelet(3, [[2 * r, 0.0], [3 * r, -bulge], [4 * r, 0.0]], (301, 401, 302, 402)),
           lanelet(4, [[4 * r, 0.0], [5 * r, 0.0], [5 * r, -4 * r], [-r, -4 * r], [-r, 0.0], [0.0, 0.0]], (302, 402, 300, 400))]
    return lanelet2.LaneletMap([], np.zeros((0, 3)), out)
