"""A CPU restatement of the ROAD WALK of the range-scan kernel (csrc/scan.hip: cells_of, road_pass, pending_add, road_range_of), operation by
operation in float32, over a grid built the way tds_map_create builds it.  It answers two questions no GPU is needed for:

  * does the walk -- which cells it looks at, when it stops -- return the ranges of the definition?  Its ranges are compared with the float32 run of
    the brute-force model (tests/range_scan_model.py: same formulas per face, no grid), and must be EQUAL;
  * how much work is it?  Passes and face tests per ray, faces per cell, and what a wavefront pays for them: the 64 rays of an agent run in
    lockstep, so a wave steps through, pass by pass, the LONGEST list walk among its lanes.

    python tools/range_scan_walk_model.py [--map town01] [--agents 24] [--rays 64] [--max-range 50] [--pend 8] [--seed 3]

Prints one JSON document.  Pure numpy and Python loops: a second or two per agent.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
f32 = np.float32
INF = f32(np.inf)


def cell_coord(v, origin, inv):
    return int(np.floor(f32(f32(v - origin) * inv)))


def build_grid(verts, faces, cell=8.0):
    """the uniform grid of tds_map_create: one entry per (cell, face whose bounding box touches the cell)"""
    cell = f32(cell)
    tri = verts[faces]
    used = verts[np.unique(faces)]
    ox, oy, inv = f32(used[:, 0].min()), f32(used[:, 1].min()), f32(1.0) / cell
    nx, ny = cell_coord(f32(used[:, 0].max()), ox, inv) + 1, cell_coord(f32(used[:, 1].max()), oy, inv) + 1
    cells = {}
    for f, t in enumerate(tri):
        cx0, cx1 = cell_coord(t[:, 0].min(), ox, inv), cell_coord(t[:, 0].max(), ox, inv)
        cy0, cy1 = cell_coord(t[:, 1].min(), oy, inv), cell_coord(t[:, 1].max(), oy, inv)
        for cy in range(cy0, cy1 + 1):
            for cx in range(cx0, cx1 + 1):
                cells.setdefault((cx, cy), []).append(f)
    t64 = tri.astype(np.float64)
    area = (t64[:, 1, 0] - t64[:, 0, 0]) * (t64[:, 2, 1] - t64[:, 0, 1]) - (t64[:, 2, 0] - t64[:, 0, 0]) * (t64[:, 1, 1] - t64[:, 0, 1])
    return dict(ox=ox, oy=oy, inv=inv, cell=cell, nx=nx, ny=ny, cells=cells, tri=tri, has_area=area != 0.0)


def line_triangle(dx, dy, p):
    w = [f32(f32(dx * p[i][1]) - f32(dy * p[i][0])) for i in range(3)]
    if all(x > 0 for x in w) or all(x < 0 for x in w):
        return None
    u = [f32(f32(dx * p[i][0]) + f32(dy * p[i][1])) for i in range(3)]
    lo, hi = INF, -INF
    for i, j in ((0, 1), (1, 2), (2, 0)):
        if w[i] != w[j] and min(w[i], w[j]) <= 0 and max(w[i], w[j]) >= 0:
            c = f32(u[i] + f32(f32(u[j] - u[i]) * f32(w[i] / f32(w[i] - w[j]))))
            lo, hi = min(lo, c), max(hi, c)
    return (lo, hi) if lo <= hi else None


def cells_of(m, v0, v1, marg, origin, n):
    lo_lim, hi_lim = f32(origin - m['cell']), f32(origin + f32(f32(n + 1) * m['cell']))
    lo = min(max(f32(min(v0, v1) - marg), lo_lim), hi_lim)
    hi = min(max(f32(max(v0, v1) + marg), lo_lim), hi_lim)
    c0 = min(max(cell_coord(lo, origin, m['inv']), 0), n - 1)
    return c0, min(max(cell_coord(hi, origin, m['inv']), c0), n - 1)


def road_walk(m, ox, oy, dx, dy, gap, max_range, pend_cap):
    """-> (range, [face tests of every pass]): road_range_of with its pending list of `pend_cap` entries"""
    marg = f32(f32(0.004) + f32(f32(1e-6) * f32(f32(abs(ox) + abs(oy)) + max_range)))
    F, prev, settled, per_pass = f32(0), None, False, []
    moves = m['nx'] + m['ny'] + 2
    for _ in range(16384):
        G = f32(F + gap)
        cx0, cx1 = cells_of(m, f32(ox + f32(dx * F)), f32(ox + f32(dx * G)), marg, m['ox'], m['nx'])
        cy0, cy1 = cells_of(m, f32(oy + f32(dy * F)), f32(oy + f32(dy * G)), marg, m['oy'], m['ny'])
        if settled and cx0 >= prev[0] and cx1 <= prev[1] and cy0 >= prev[2] and cy1 <= prev[3]:
            break
        if prev is None or (cx0, cy0) != (prev[0], prev[2]):
            moves -= 1
            if moves < 0:
                break
        start, pend, dropped, tests = F, [], INF, 0
        for cy in range(cy0, cy1 + 1):
            for cx in range(cx0, cx1 + 1):
                for f in m['cells'].get((cx, cy), ()):
                    tests += 1
                    t = m['tri'][f]
                    r = line_triangle(dx, dy, [(f32(t[i][0] - ox), f32(t[i][1] - oy)) for i in range(3)])
                    if r is None:
                        continue
                    a, b = max(r[0], f32(0)), min(r[1], max_range)
                    if not a <= b or not b > F or not m['has_area'][f]:
                        continue
                    if a <= f32(F + gap):
                        F = b
                    elif len(pend) < pend_cap:
                        pend.append((a, b))
                    elif pend_cap and a < max(p[0] for p in pend):
                        im = max(range(pend_cap), key=lambda i: pend[i][0])
                        dropped = min(dropped, pend[im][0])
                        pend[im] = (a, b)
                    else:
                        dropped = min(dropped, a)
        grew, rounds = bool(pend), 0
        while grew and rounds <= pend_cap:
            grew, rounds = False, rounds + 1
            for a, b in pend:
                if a <= f32(F + gap) and b > F:
                    F, grew = b, True
        per_pass.append(tests)
        settled, prev = bool(f32(F + gap) < dropped), (cx0, cx1, cy0, cy1)
        if not F > start or F >= max_range:
            break
    return min(F, max_range), per_pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--map', default='town01', choices=['town01', 'town02'])
    ap.add_argument('--agents', type=int, default=24)
    ap.add_argument('--rays', type=int, default=64)
    ap.add_argument('--max-range', type=float, default=50.0)
    ap.add_argument('--gap', type=float, default=0.02)
    ap.add_argument('--pend', type=int, default=8, help='entries of the per-lane pending list (scan.hip: PEND); 0: none')
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    import range_scan_model as rm
    from test_range_scan_model import origins_on_road, town
    verts, faces, road = town(args.map)
    m = build_grid(verts, faces)
    xy, psi = origins_on_road(verts, faces[road], args.agents, seed=args.seed)
    R, max_range, gap = args.rays, f32(args.max_range), f32(args.gap)
    off = (-np.pi + 2 * np.pi * (np.arange(R) + 0.5) / R).astype(f32)
    unequal, lane_tests, lane_passes, wave_entries, wave_passes, ranges = 0, [], [], [], [], []
    for a in range(args.agents):
        ang = (psi[a] + off).astype(f32)
        d = np.stack([np.cos(ang), np.sin(ang)], -1).astype(f32)
        want = rm.road_ranges(verts, faces, xy[a], d, args.max_range, args.gap, np.float32)
        per = []
        for k in range(R):
            got, per_pass = road_walk(m, xy[a][0], xy[a][1], d[k, 0], d[k, 1], gap, max_range, args.pend)
            unequal += int(got != want[k])
            ranges.append(float(got))
            per.append(per_pass)
        lane_tests += [sum(p) for p in per]
        lane_passes += [len(p) for p in per]
        for w0 in range(0, R, 64):                                   # the lanes of a wave run pass i together: it costs the longest list walk
            lanes = per[w0:w0 + 64]
            n = max(len(p) for p in lanes)
            wave_passes.append(n)
            wave_entries.append(sum(max((p[i] if i < len(p) else 0) for p in lanes) for i in range(n)))
    sizes = np.array([len(v) for v in m['cells'].values()])
    print(json.dumps(dict(
        map=args.map, agents=args.agents, rays_per_agent=R, max_range=args.max_range, gap_tolerance=args.gap, pending_entries=args.pend, seed=args.seed,
        grid=dict(nx=m['nx'], ny=m['ny'], cells_with_faces=int(len(sizes)), faces_per_cell_mean=round(float(sizes.mean()), 1),
                  faces_per_cell_median=int(np.median(sizes)), faces_per_cell_max=int(sizes.max())),
        rays=len(ranges), rays_unequal_to_the_float32_model=unequal, mean_road_range_m=round(float(np.mean(ranges)), 2),
        per_ray=dict(passes_mean=round(float(np.mean(lane_passes)), 2), passes_max=int(max(lane_passes)), face_tests_mean=round(float(np.mean(lane_tests)), 1),
                     face_tests_max=int(max(lane_tests))),
        per_wave=dict(passes_mean=round(float(np.mean(wave_passes)), 2), passes_max=int(max(wave_passes)),
                      list_entries_stepped_through_mean=round(float(np.mean(wave_entries)), 1),
                      over_the_mean_lane=round(float(np.mean(wave_entries)) / float(np.mean(lane_tests)), 2))), indent=1))
    return 1 if unequal else 0


if __name__ == '__main__':
    sys.exit(main())
