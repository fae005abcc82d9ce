"""The CPU restatement of the scan kernel's road walk (tools/range_scan_walk_model.py: the cells it looks at, its pending list, when it stops)
returns the ranges of the brute-force model run in float32 -- exactly, since both evaluate the same formulas per face.  A small sample here; the
tool itself reports 1 536 rays (profiles/range_scan_walk_model.json)."""
import os
import sys

import numpy as np
import pytest

import range_scan_model as rm
from test_range_scan_model import origins_on_road, town

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))


@pytest.mark.parametrize('name, pend', [('town01', 8), ('town02', 8), ('town02', 0), ('town01', 2)])
def test_the_walk_returns_the_models_float32_ranges(name, pend):
    import range_scan_walk_model as wm
    verts, faces, road = town(name)
    grid = wm.build_grid(verts, faces)
    xy, psi = origins_on_road(verts, faces[road], 3, seed=17)
    # one origin outside the grid, one a hair outside the road
    xy = np.concatenate([xy, np.array([[-500.0, -500.0], [verts[:, 0].min() - 0.01, verts[:, 1].mean()]], np.float32)])
    psi = np.concatenate([psi, np.zeros(2, np.float32)])
    R, passes = 12, []
    for a in range(len(xy)):
        ang = (psi[a] + np.linspace(-np.pi, np.pi, R, endpoint=False)).astype(np.float32)
        d = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)
        want = rm.road_ranges(verts, faces, xy[a], d, 60.0, 0.02, np.float32)
        for k in range(R):
            got, per_pass = wm.road_walk(grid, xy[a][0], xy[a][1], d[k, 0], d[k, 1], np.float32(0.02), np.float32(60.0), pend)
            assert got == want[k], (name, a, k, got, want[k])
            passes.append(len(per_pass))
    assert max(passes) < 64
