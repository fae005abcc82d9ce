"""
The yardstick of the range-scan kernel (csrc/scan.hip, Simulator.compute_range_scan): a numpy model of the DEFINITION (DESIGN.md "K5"), brute
force over ALL faces and ALL entities -- no grid, no cell walk, so it cannot share a bug with the kernel's -- evaluated in float64 (or, for the
error table of tests/test_range_scan_model.py, in float32) on the same float32 inputs the kernel gets, [sin, cos] included.

One scene per call:
    verts (V, 2), faces (F, 3)           the road mesh (None / F = 0: no road part)
    boxes (E, 5) [x, y, length, width, psi], sc (E, 2) [sin, cos] of psi, present (E,)     exposed agents first
    ray_sc (A, R, 2) [sin, cos] of every ray of the A exposed agents
"""
import numpy as np


def positive_area(verts, faces):
    """(F,) bool: faces that count as road -- non-zero area, in float64 on the float32 vertices (padding faces [0, 0, 0] drop out here)"""
    t = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    return ((t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 2, 0] - t[:, 0, 0]) * (t[:, 1, 1] - t[:, 0, 1])) != 0.0


def face_intervals(tri, origin, d, max_range, dtype=np.float64):
    """For R rays from one origin: where does each ray meet each closed triangle?  tri (F, 3, 2), origin (2,), d (R, 2) unit vectors [dx, dy].
    Returns (ray index, face index, a, b) of the non-empty intervals [a, b] within [0, max_range].
    With the vertices relative to the origin, u = p . d runs along the ray and w = d x p is the signed distance from its line; an edge whose
    end points lie on different sides of the line (or on it) crosses it at u_i + (u_j - u_i) * w_i / (w_i - w_j)."""
    dt = np.dtype(dtype).type
    p = tri.astype(dtype) - np.asarray(origin, dtype)                    # F x 3 x 2
    dx, dy = d[:, 0].astype(dtype)[:, None, None], d[:, 1].astype(dtype)[:, None, None]
    w = dx * p[None, :, :, 1] - dy * p[None, :, :, 0]                    # R x F x 3
    touch = ~((w > 0).all(-1) | (w < 0).all(-1))
    r, f = np.nonzero(touch)
    w = w[r, f]                                                          # n x 3
    u = dx[r, 0] * p[f][:, :, 0] + dy[r, 0] * p[f][:, :, 1]
    lo, hi = np.full(len(r), np.inf, dtype), np.full(len(r), -np.inf, dtype)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        wi, wj, ui, uj = w[:, i], w[:, j], u[:, i], u[:, j]
        ok = (wi != wj) & (np.minimum(wi, wj) <= 0) & (np.maximum(wi, wj) >= 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            c = ui + (uj - ui) * (wi / (wi - wj))
        lo = np.where(ok, np.minimum(lo, c), lo)
        hi = np.where(ok, np.maximum(hi, c), hi)
    a, b = np.maximum(lo, dt(0)), np.minimum(hi, dt(max_range))
    keep = a <= b
    return r[keep], f[keep], a[keep], b[keep]


def fixed_point(a, b, gap, dtype=np.float64):
    """the least fixed point of F <- max{b_f : a_f <= F + gap} from F = 0, over the intervals of ONE ray"""
    dt = np.dtype(dtype).type
    F, gap = dt(0), dt(gap)
    for i in np.argsort(a, kind='stable'):
        if not a[i] <= dt(F + gap):
            break
        if b[i] > F:
            F = b[i]
    return F


def road_ranges(verts, faces, origin, d, max_range, gap_tolerance, dtype=np.float64, gaps=None):
    """(R,) road ranges of R rays from `origin` (or (len(gaps), R) for several tolerances at once: the sensitivity of a ray to the threshold)"""
    verts, faces = np.asarray(verts, np.float32)[:, :2], np.asarray(faces, np.int64)
    faces = faces[positive_area(verts, faces)]
    tri = verts[faces]
    # every face is looked at: those whose bounding box is out of the rays' reach are dropped by a test of the box, a metre to spare
    o = np.asarray(origin, np.float64)
    reach = float(max_range) + 1.0
    near = ((tri[..., 0].max(1) >= o[0] - reach) & (tri[..., 0].min(1) <= o[0] + reach) & (tri[..., 1].max(1) >= o[1] - reach) &
            (tri[..., 1].min(1) <= o[1] + reach))
    r, f, a, b = face_intervals(tri[near], np.asarray(origin, np.float32), np.asarray(d, np.float32), max_range, dtype)
    order = np.argsort(r, kind='stable')
    r, a, b = r[order], a[order], b[order]
    start = np.searchsorted(r, np.arange(len(d) + 1))
    gl = [gap_tolerance] if gaps is None else list(gaps)
    out = np.zeros((len(gl), len(d)), dtype)
    for k in range(len(d)):
        s, e = start[k], start[k + 1]
        for g, gap in enumerate(gl):
            out[g, k] = min(fixed_point(a[s:e], b[s:e], gap, dtype), np.dtype(dtype).type(max_range))
    return out[0] if gaps is None else out


def agent_ranges(boxes, sc, present, a, d, max_range, dtype=np.float64):
    """rays d (R, 2) of exposed agent `a` against the rectangles of all OTHER present entities: (t (R, E) with inf for a miss)"""
    boxes, sc = np.asarray(boxes, np.float32).astype(dtype), np.asarray(sc, np.float32).astype(dtype)
    d = np.asarray(d, np.float32).astype(dtype)
    E = len(boxes)
    rx, ry = boxes[a, 0] - boxes[:, 0], boxes[a, 1] - boxes[:, 1]         # the origin relative to every centre
    s, c = sc[:, 0], sc[:, 1]
    lx, ly = rx * c + ry * s, ry * c - rx * s                            # ... in every rectangle's frame
    ex = d[:, 0, None] * c + d[:, 1, None] * s                           # R x E
    ey = d[:, 1, None] * c - d[:, 0, None] * s
    t0, t1 = np.zeros_like(ex), np.full_like(ex, np.inf)
    ok = np.ones(ex.shape, bool)
    for e, l, h in ((ex, lx, boxes[:, 2] / 2), (ey, ly, boxes[:, 3] / 2)):
        par = e == 0
        with np.errstate(divide='ignore', invalid='ignore'):
            u, v = (-h - l) / e, (h - l) / e
        ok &= np.where(par, np.abs(l) <= h, True)
        t0 = np.where(par, t0, np.maximum(t0, np.minimum(u, v)))
        t1 = np.where(par, t1, np.minimum(t1, np.maximum(u, v)))
    ok &= t0 <= t1
    ok &= np.asarray(present, bool)[None, :]
    ok[:, a] = False
    return np.where(ok, t0, np.inf)


def hit_of(t, agents, road, max_range):
    """the hit code of one ray from its entity distances t (E,), its two ranges and max_range"""
    if agents < max_range and agents <= road:
        return int(np.argmin(t))                                         # (the lowest index among equals)
    if road < max_range and road < agents:
        return -2
    return -1


def range_scan(verts, faces, boxes, sc, present, ray_sc, max_range, gap_tolerance, dtype=np.float64, with_agents=True, sensitivity=False):
    """-> dict(agents (A, R), road (A, R), hit (A, R) int32, t (A, R, E) every entity's distance (inf: missed)) and, with sensitivity=True,
    road_lo / road_hi: the road ranges at gap_tolerance * (1 -/+ 1e-3) -- a ray whose two differ is threshold-sensitive"""
    ray_sc = np.asarray(ray_sc, np.float32)
    A, R = ray_sc.shape[:2]
    E = len(boxes)
    dt = np.dtype(dtype).type
    present = np.asarray(present, bool)
    has_road = faces is not None and len(faces) > 0
    out = dict(agents=np.full((A, R), dt(max_range), dtype), road=np.full((A, R), dt(max_range), dtype), hit=np.full((A, R), -1, np.int32),
               t=np.full((A, R, E), np.inf, dtype))
    if sensitivity:
        out['road_lo'], out['road_hi'] = out['road'].copy(), out['road'].copy()
    for a in range(A):
        if not present[a]:
            continue
        d = ray_sc[a][:, ::-1]                                           # [cos, sin] = the direction
        if with_agents:
            t = agent_ranges(boxes, sc, present, a, d, max_range, dtype)
            out['t'][a] = t
            out['agents'][a] = np.minimum(t.min(1) if E else np.inf, dt(max_range))
        if has_road:
            origin = np.asarray(boxes, np.float32)[a, :2]
            if sensitivity:
                g = gap_tolerance
                out['road'][a], out['road_lo'][a], out['road_hi'][a] = road_ranges(verts, faces, origin, d, max_range, g, dtype, gaps=(g, g * (1 - 1e-3), g * (1 + 1e-3)))
            else:
                out['road'][a] = road_ranges(verts, faces, origin, d, max_range, gap_tolerance, dtype)
        for k in range(R):
            out['hit'][a, k] = hit_of(out['t'][a, k], out['agents'][a, k], out['road'][a, k], dt(max_range))
    return out
