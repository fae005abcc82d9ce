"""Brute-force numpy model of time to collision (include/tdship.h "K9"): the float32 inputs widened to float64, the operations of
the definition in its order, each rounded once -- numpy arithmetic does not contract --, one rounding to float32 at the end, so the kernel
(csrc/ttc.hip) and the host build of csrc/tds_ttc.h must equal it bit for bit.  `stepped` is the independent yardstick of
tests/test_ttc_model.py: rectangle overlap tested at fixed time steps."""
import numpy as np

import neighbors_model as nm

MAX_K, MAX_ENTITIES = 32, 1024
F32, F64 = np.float32, np.float64


def pair_interval(a, e, margin=0.0):
    """one observer a = (x, y, l, w, s, c, v) against the entities e = the same seven as arrays of n, all float64 and finite, by the definition
    -> (possible (n,) bool: no axis with w == 0 separates the pair, lo (n,), hi (n,))"""
    xa, ya, la, wa, sa, ca, va = (F64(v) for v in a)
    xe, ye, le, we, se, ce, ve = (np.asarray(v, F64) for v in e)
    margin = F64(margin)
    hla, hwa = F64(0.5) * la + margin, F64(0.5) * wa + margin
    hle, hwe = F64(0.5) * le, F64(0.5) * we
    dx, dy = xe - xa, ye - ya
    rvx, rvy = ve * ce - va * ca, ve * se - va * sa
    n = dx.shape
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    possible = np.ones(n, bool)
    with np.errstate(all='ignore'):
        for nx, ny in ((np.full(n, ca), np.full(n, sa)), (np.full(n, -sa), np.full(n, ca)), (ce, se), (-se, ce)):
            p = dx * nx + dy * ny
            w = rvx * nx + rvy * ny
            R = hla * np.abs(ca * nx + sa * ny) + hwa * np.abs(ca * ny - sa * nx) + hle * np.abs(ce * nx + se * ny) + hwe * np.abs(ce * ny - se * nx)
            still = w == 0
            possible &= ~(still & (np.abs(p) > R))
            ws = np.where(still, 1.0, w)
            t0, t1 = (-R - p) / ws, (R - p) / ws
            swap = t0 > t1
            t0, t1 = np.where(swap, t1, t0), np.where(swap, t0, t1)
            lo = np.where(~still & (t0 > lo), t0, lo)
            hi = np.where(~still & (t1 < hi), t1, hi)
    return possible, lo, hi


def pair_ttc(a, e, horizon, margin=0.0):
    """-> (candidate (n,) bool, ttc (n,) float32: the time of a candidate, +inf elsewhere)"""
    possible, lo, hi = pair_interval(a, e, margin)
    cand = possible & (lo <= hi) & (hi >= 0) & (lo <= F64(F32(horizon)))
    with np.errstate(over='ignore'):
        t = np.where(lo > 0, lo, 0.0).astype(F32)
    return cand, np.where(cand, t, F32(np.inf))


def values(boxes, sc, speed, b):
    """the seven float32 values of every entity of scene b, widened: x, y, l, w, s, c, v"""
    return [boxes[b, :, 0].astype(F64), boxes[b, :, 1].astype(F64), boxes[b, :, 2].astype(F64), boxes[b, :, 3].astype(F64),
            sc[b, :, 0].astype(F64), sc[b, :, 1].astype(F64), speed[b].astype(F64)]


def time_to_collision(boxes, sc, speed, present, n_exposed, k, horizon, margin=0.0, visible=None):
    """boxes (B,E,5), sc (B,E,2), speed (B,E), present (B,E), visible None or (B,A,E) -> ttc (B,A,k) float32, index (B,A,k) int32"""
    boxes, sc, speed = np.asarray(boxes, F32), np.asarray(sc, F32), np.asarray(speed, F32)
    present = np.asarray(present).astype(bool)
    B, E = boxes.shape[:2]
    A, K = int(n_exposed), int(k)
    assert 1 <= K <= MAX_K and A <= E <= MAX_ENTITIES and F32(horizon) >= 0 and np.isfinite(F32(margin))
    ttc = np.full((B, A, K), np.inf, F32)
    index = np.full((B, A, K), -1, np.int32)
    ents = np.arange(E)
    for b in range(B):
        v = values(boxes, sc, speed, b)
        finite = np.all([np.isfinite(q) for q in v], 0)
        usable = present[b] & finite
        safe = [np.where(finite, q, 0.0) for q in v]                         # the values of a non-finite entity are never looked at
        for a in range(A):
            if not usable[a]:
                continue
            cand, t = pair_ttc([q[a] for q in safe], safe, horizon, F32(margin))
            cand &= usable & (ents != a)
            if visible is not None:
                cand &= np.asarray(visible[b, a]) != 0
            who = ents[cand]
            who = who[np.lexsort((who, t[cand].view(np.uint32)))][:K]       # by the bits of ttc, equal bits by the lower entity index
            ttc[b, a, :len(who)] = t[who]
            index[b, a, :len(who)] = who
    return ttc, index


# ---- the yardstick: overlap of the two rectangles at fixed time steps, float64, np.sin / np.cos of the heading -------------------------------------
def overlap(xa, ya, la, wa, pa, xe, ye, le, we, pe):
    """whether two rectangles (centre, length, width, heading; arrays of n) touch: the separating-axis test on their corners -> (n,) bool"""
    def corners(x, y, l, w, psi):
        c, s = np.cos(psi), np.sin(psi)
        return [(x + c * hx - s * hy, y + s * hx + c * hy) for hx, hy in ((l / 2, w / 2), (l / 2, -w / 2), (-l / 2, -w / 2), (-l / 2, w / 2))]
    ca, ce = corners(xa, ya, la, wa, pa), corners(xe, ye, le, we, pe)
    touch = np.ones(np.shape(xa), bool)
    for psi in (pa, pe):
        for ax, ay in ((np.cos(psi), np.sin(psi)), (-np.sin(psi), np.cos(psi))):
            qa = np.stack([x * ax + y * ay for x, y in ca])
            qe = np.stack([x * ax + y * ay for x, y in ce])
            touch &= ~((qa.max(0) < qe.min(0)) | (qe.max(0) < qa.min(0)))
    return touch


def stepped(pairs, horizon=5.0, step=0.01):
    """pairs (n, 2, 6) [x, y, l, w, psi, v]: the first multiple of `step` within the horizon at which the rectangles touch, in float64 -> (n,), +inf
    where none does"""
    q = np.asarray(pairs, F64)
    (xa, ya, la, wa, pa, va), (xe, ye, le, we, pe, ve) = (q[:, 0].T, q[:, 1].T)
    first = np.full(len(q), np.inf)
    for i in range(int(round(horizon / step)) + 1):
        t = i * step
        hit = overlap(xa + va * np.cos(pa) * t, ya + va * np.sin(pa) * t, la, wa, pa, xe + ve * np.cos(pe) * t, ye + ve * np.sin(pe) * t, le, we, pe)
        first = np.where(hit & np.isinf(first), t, first)
    return first


def random_pairs(seed=0, n=4000, side=60.0):
    """the pairs of the check against time stepping: (n, 2, 6) float32 [x, y, l, w, psi, v] in a square of `side` metres, speeds 0 .. 15 m/s"""
    g = np.random.default_rng(seed)
    return np.concatenate([g.uniform(0, side, (n, 2, 2)), g.uniform(3.5, 6.0, (n, 2, 1)), g.uniform(1.6, 2.4, (n, 2, 1)), g.uniform(-np.pi, np.pi, (n, 2, 1)),
                           g.uniform(0, 15, (n, 2, 1))], -1).astype(F32)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def scene(rows):
    """rows of (x, y, l, w, psi, v, present) per scene -> dict(boxes, sc, speed, present); the headings are multiples of pi / 2 given in quarter
    turns, so that [sin, cos] are exactly 0 and +-1"""
    r = np.asarray(rows, F64)
    quarter = r[..., 4].astype(int) % 4
    sc = np.stack([np.array([0.0, 1.0, 0.0, -1.0])[quarter], np.array([1.0, 0.0, -1.0, 0.0])[quarter]], -1).astype(F32)
    boxes = np.concatenate([r[..., :4], (r[..., 4:5] * (np.pi / 2))], -1).astype(F32)
    return dict(boxes=boxes, sc=sc, speed=r[..., 5].astype(F32), present=r[..., 6] != 0)


DEFINITION_HORIZON = 3.0
BEYOND = float(np.nextafter(F32(34.0), F32(35.0)))       # a float32 step past the gap that closes in exactly 3 s


def definition_cases():
    """B = 2, A = 3, E = 6, to be asked for K = 4 within DEFINITION_HORIZON = 3 s, margin 0 -> dict(boxes, sc, speed, present).  All boxes are
    4 x 2 m, all headings quarter turns, so every time is exact.
    scene 0: observer 0 at the origin drives east at 10 m/s.  Entity 1, 50 m ahead, comes head-on at 10 m/s: 46 m gap, 2.3 s.  Entity 2, 20 m
             behind it on the next lane (y = 3.5), same speed, same heading: never.  Entity 3 crosses from the south at right angles and reaches
             the lane at 2.3 s too (the tie: 1 comes first).  Entity 4 stands 34 m ahead: gap 30 m, contact at exactly 3 s = the horizon (in).
             Entity 5 stands a float32 step further: out.  Observer 0 has 3 candidates for 4 slots.  Observer 1, the oncoming one, meets
             the two standing ones first, the further one a float32 step sooner, then 0 and 3 in a tie.  Observer 2 meets nobody.
    scene 1: observer 0 is absent (an empty row, and nobody's candidate); observer 1 and observer 2 overlap (0 s); entity 3 has a NaN pose (never
             a candidate); entity 4 is an absent NPC on top of them; entity 5 drives away."""
    s0 = [(0, 0, 4, 2, 0, 10, 1), (50, 0, 4, 2, 2, 10, 1), (-20, 3.5, 4, 2, 0, 10, 1), (26, -26, 4, 2, 1, 10, 1), (34, 0, 4, 2, 0, 0, 1),
          (BEYOND, 0, 4, 2, 0, 0, 1)]
    s1 = [(1, 1, 4, 2, 0, 5, 0), (0, 0, 4, 2, 0, 5, 1), (3, 1, 4, 2, 1, 5, 1), (np.nan, 2, 4, 2, 0, 1, 1), (1, 0.5, 4, 2, 0, 3, 0), (30, 0, 4, 2, 0, 20, 1)]
    return scene([s0, s1])


#: the outputs of definition_cases() at K = 4, horizon 3, margin 0, by hand from the definition
INF = float('inf')
DEFINITION_INDEX = [[[1, 3, 4, -1], [5, 4, 0, 3], [-1, -1, -1, -1]], [[-1, -1, -1, -1], [2, -1, -1, -1], [1, -1, -1, -1]]]
DEFINITION_TTC = [[[2.3, 2.3, 3.0, INF], [(46.0 - BEYOND) / 10.0, 1.2, 2.3, 2.3], [INF] * 4], [[INF] * 4, [0.0, INF, INF, INF], [0.0, INF, INF, INF]]]


def random_scenes(seed, B, A, E, side=None, duplicates=0.05, absent=0.1):
    """the generator of neighbors_model in a square whose side grows with the number of entities, so that a fair share of the observers has
    something on its way whatever E is (side: 7 m * sqrt(E), at least 20 m); a share stands exactly on another entity (time 0), a share is
    absent, and entity E - 1 of every scene has a NaN speed"""
    side = max(20.0, 7.0 * float(np.sqrt(E))) if side is None else side
    s = nm.random_scenes(seed, B, A, E, side=side, duplicates=duplicates, absent=absent)
    s['speed'][:, E - 1] = np.nan
    return s


#: the random scenes the device tests run, name -> (seed, B, A, E[, side]): tests/test_ttc_model.py asserts on each that at least a quarter of the present
#: observers has a finite time within 3 s, that at least one time is 0 and at least one above 0 (E1024 is dense: both observers have 32 candidates)
SCENES = {'E6': (107, 2, 5, 6), 'E64': (164, 2, 5, 64), 'E65': (165, 2, 5, 65), 'E130': (230, 2, 5, 130), 'E1024': (1109, 1, 2, 1024, 120.0),
          'mask40': (140, 3, 6, 40), 'mask100': (200, 2, 3, 100)}
COVERAGE_HORIZON = 3.0


def scenes(name):
    seed, B, A, E = SCENES[name][:4]
    return random_scenes(seed, B, A, E, *SCENES[name][4:]), A
