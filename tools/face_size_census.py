#!/usr/bin/env python3
"""Which faces the fused rasteriser's per-face cost is spent on: a CPU census of the bench's views (numpy, no GPU).
Cameras are the bench's agents (bench.synth_agents, seed 1234: position and heading of each agent), fov 35 m, 256 x 256, Town01.  Per view the
faces go through the reference's projection trunc(-R(v - cam) * res / fov + res / 2), the bounding-box reject against the image and the 1.05
trim (a face stays when one of its vertices lies in the 1.05 x view), as the kernel's scan does.  Reported per view:
  faces by category; the distribution of the pixel height yb - yt; the share of faces and of row items (4-row items of one part between the
  vertex rows, process_batch_bits' CHUNK) by world diameter (longest vertex distance); the share of "small" faces (all vertices inside the image,
  yb - yt <= ROWS - 1) per diameter class; grid entries scanned against accepted (one entry per face and cell its box touches, rows of cells
  under the rotated 1.05 x view, the owner rule not modelled: an upper bound of what the scan offers).
   python tools/face_size_census.py [--views 300] [--res 256] [--fov 35] [--rows 7] [--cell 0] [--town 1] [--json OUT]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CHUNK = 4            # rows per item of the scan conversion (TDS_FCHUNK of csrc/raster.hip)


def project(verts, cam_xy, psi, res, fov):
    """pixel coordinates (int32, truncated) and their float values, in float32 as the kernel and the oracle compute them"""
    f32 = np.float32
    s, c = f32(np.sin(f32(psi))), f32(np.cos(f32(psi)))
    x, y = verts[:, 0].astype(f32) - f32(cam_xy[0]), verts[:, 1].astype(f32) - f32(cam_xy[1])
    scale = f32(2.0) / f32(fov)
    rx, ry = (-(c * x + s * y)) * scale, (-((-s) * x + c * y)) * scale
    rx, ry = rx * f32(res) / f32(2) + f32(res) / f32(2), ry * f32(res) / f32(2) + f32(res) / f32(2)
    return np.trunc(rx).astype(np.int64), np.trunc(ry).astype(np.int64), rx, ry


def grid_entries(bmin, bmax, origin, cell):
    """entries per cell: every face in all the cells its bounding box touches"""
    lo = np.floor((bmin - origin) / cell).astype(np.int64)
    hi = np.floor((bmax - origin) / cell).astype(np.int64)
    nx, ny = int(hi[:, 0].max()) + 1, int(hi[:, 1].max()) + 1
    count = np.zeros((ny, nx), np.int64)
    for (x0, y0), (x1, y1) in zip(lo, hi):
        count[y0:y1 + 1, x0:x1 + 1] += 1
    return count


def scanned(count, origin, cell, cam_xy, psi, fov):
    """entries of the cells in the per-row ranges under the rotated 1.05 x view"""
    h = 0.5 * fov * 1.05
    c, s = np.cos(psi), np.sin(psi)
    Q = np.array([[-h, -h], [-h, h], [h, h], [h, -h]]) @ np.array([[c, -s], [s, c]]).T + cam_xy
    ny, nx = count.shape
    cy0, cy1 = int(np.floor((Q[:, 1].min() - origin[1]) / cell)), int(np.floor((Q[:, 1].max() - origin[1]) / cell))
    total = 0
    for cy in range(max(cy0, 0), min(cy1, ny - 1) + 1):
        ya, yb = origin[1] + cy * cell, origin[1] + (cy + 1) * cell
        xs = []
        for k in range(4):
            (x0, y0), (x1, y1) = Q[k], Q[(k + 1) % 4]
            if ya <= y0 <= yb:
                xs.append(x0)
            for yl in (ya, yb):
                if (y0 - yl) * (y1 - yl) <= 0 and y1 != y0:
                    xs.append(x0 + (yl - y0) / (y1 - y0) * (x1 - x0))
        if xs:
            a, b = int(np.floor((min(xs) - origin[0]) / cell)), int(np.floor((max(xs) - origin[0]) / cell))
            total += int(count[cy, max(a, 0):min(b, nx - 1) + 1].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=300)
    ap.add_argument('--res', type=int, default=bench.RES)
    ap.add_argument('--fov', type=float, default=bench.FOV)
    ap.add_argument('--rows', type=int, default=7, help='ROWS of the on-lane path: a face is small when yb - yt <= ROWS - 1 and all its vertices are inside the image')
    ap.add_argument('--cell', type=float, default=0.0, help='grid cell in metres (0: 0.65 fov, the library default at the bench fov)')
    ap.add_argument('--town', type=int, default=1, choices=(1, 2))
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    verts, faces, vcat, cats = bench.load_town01() if args.town == 1 else bench.load_town02()
    verts = verts.astype(np.float64)
    A = 64
    B = (args.views + A - 1) // A
    state = bench.synth_agents(B, A, verts[vcat == cats.index('road')].astype(np.float32), args.seed)[0].reshape(-1, 4)[:args.views]
    res, fov = args.res, args.fov
    P = verts[faces]                                                    # F, 3, 2
    fcat = vcat[faces[:, 0]]
    diam = np.sqrt(np.max([((P[:, i] - P[:, j]) ** 2).sum(-1) for i, j in ((0, 1), (1, 2), (2, 0))], axis=0))
    cell = args.cell or 0.65 * fov
    origin = verts.min(0)
    count = grid_entries(P.min(1), P.max(1), origin, cell)
    classes = [0.55, 0.7, 0.8, (args.rows - 1) * fov / res, 1.0, 1.5, 1e9]
    acc_cat = np.zeros(len(cats), np.int64)
    height_hist = np.zeros(res + 2, np.int64)
    cls_faces, cls_items, cls_small = np.zeros(len(classes), np.int64), np.zeros(len(classes), np.int64), np.zeros(len(classes), np.int64)
    tot = dict(accepted=0, items=0, small=0, small_items=0, inside=0, scanned=0)
    med = {c: [] for c in cats}
    small_heights = []
    for cam in state:
        px, py, fx, fy = project(verts, cam[:2], cam[2], res, fov)
        X, Y = px[faces], py[faces]
        hit = ~((X.max(1) < 0) | (X.min(1) >= res) | (Y.max(1) < 0) | (Y.min(1) >= res))
        lo, hi = -0.025 * res, 1.025 * res
        vin = (np.minimum(fx, fy) > lo) & (np.maximum(fx, fy) < hi)
        acc = hit & vin[faces].any(1)
        X, Y, d, fc = X[acc], Y[acc], diam[acc], fcat[acc]
        ys = np.sort(Y, 1)
        yt, ym, yb = ys[:, 0], ys[:, 1], ys[:, 2]
        n1 = np.maximum(0, np.minimum(ym - 1, res - 1) - np.maximum(yt + 1, 0) + 1)
        n2 = np.maximum(0, np.minimum(yb - 1, res - 1) - np.maximum(ym + 1, 0) + 1)
        items = (n1 + CHUNK - 1) // CHUNK + (n2 + CHUNK - 1) // CHUNK
        inside = ((X >= 0) & (X < res) & (Y >= 0) & (Y < res)).all(1)
        small = inside & (yb - yt <= args.rows - 1)
        tot['accepted'] += len(d); tot['items'] += int(items.sum()); tot['small'] += int(small.sum()); tot['inside'] += int(inside.sum())
        tot['small_items'] += int(items[small].sum())
        tot['scanned'] += scanned(count, origin, cell, cam[:2].astype(np.float64), float(cam[2]), fov)
        acc_cat += np.bincount(fc, minlength=len(cats))
        height_hist += np.bincount(np.clip(yb - yt, 0, res + 1), minlength=res + 2)
        for k, c in enumerate(cats):
            if (fc == k).any():
                med[c].append((float(np.median((X.max(1) - X.min(1))[fc == k])), float(np.median((yb - yt)[fc == k]))))
        for k, t in enumerate(classes):
            sel = d <= t
            cls_faces[k] += int(sel.sum()); cls_items[k] += int(items[sel].sum()); cls_small[k] += int((small & sel).sum())
        small_heights.append((yb - yt)[d <= 0.8])
    n = len(state)
    out = {'views': n, 'res': res, 'fov': fov, 'rows': args.rows, 'cell_m': cell, 'town': args.town,
           'accepted_per_view': tot['accepted'] / n, 'row_items_per_view': tot['items'] / n, 'scanned_entries_per_view': tot['scanned'] / n,
           'faces_per_view_by_category': {c: acc_cat[k] / n for k, c in enumerate(cats) if acc_cat[k]},
           'median_px_width_height_by_category': {c: [float(np.median([m[0] for m in v])), float(np.median([m[1] for m in v]))] for c, v in med.items() if v},
           'small_share_of_faces': tot['small'] / tot['accepted'], 'small_share_of_row_items': tot['small_items'] / max(tot['items'], 1),
           'all_vertices_inside_share': tot['inside'] / tot['accepted'],
           'height_share': {str(h): height_hist[h] / tot['accepted'] for h in range(0, 13)},
           'height_share_above_12': height_hist[13:].sum() / tot['accepted'],
           'by_world_diameter': [{'diameter_le_m': (None if t > 1e8 else round(float(t), 4)), 'share_of_faces': cls_faces[k] / tot['accepted'],
                                  'share_of_row_items': cls_items[k] / max(tot['items'], 1), 'small_share_within': cls_small[k] / max(cls_faces[k], 1)}
                                 for k, t in enumerate(classes)]}
    sh = np.concatenate(small_heights)
    out['height_of_faces_le_0.8m'] = {'p50': float(np.percentile(sh, 50)), 'p99': float(np.percentile(sh, 99)), 'max': int(sh.max())} if len(sh) else None
    print(json.dumps(out, indent=1, default=float))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1, default=float)
            f.write('\n')


if __name__ == '__main__':
    main()
