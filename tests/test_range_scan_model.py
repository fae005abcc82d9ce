"""The float64 model of the range scan (tests/range_scan_model.py) against distances computed by hand, and the table the GPU tolerance comes
from: the same model run in float32 against float64 on the golden Town01 / Town02 meshes (CPU only)."""
import math
import os

import numpy as np
import pytest

import range_scan_model as rm
from conftest import GOLDEN

SQUARE_V = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float32)
SQUARE_F = np.array([[0, 1, 2], [0, 2, 3]])


def rays(angles):
    a = np.asarray(angles, np.float32)
    return np.stack([np.sin(a), np.cos(a)], -1).astype(np.float32)


def exact_rays(dirs):
    """[sin, cos] of directions given as exact (dx, dy) unit vectors"""
    return np.array([[dy, dx] for dx, dy in dirs], np.float32)


def road_only(origin, ray_sc, verts=SQUARE_V, faces=SQUARE_F, max_range=100.0, gap=0.02):
    box = np.array([[origin[0], origin[1], 4.0, 2.0, 0.0]], np.float32)
    return rm.range_scan(verts, faces, box, np.array([[0.0, 1.0]], np.float32), [True], ray_sc[None], max_range, gap)


def test_square_road_along_axes_and_diagonals():
    out = road_only((2.0, 3.0), exact_rays([(1, 0), (-1, 0), (0, 1), (0, -1)]))
    assert np.allclose(out['road'][0], [8.0, 2.0, 7.0, 3.0], atol=1e-12)
    assert (out['hit'][0] == -2).all() and (out['agents'][0] == 100.0).all()
    d = out = road_only((2.0, 3.0), rays([math.pi / 4, 3 * math.pi / 4, -3 * math.pi / 4, -math.pi / 4]))
    # towards (+,+): the top edge, 7 up; (-,+): the left edge, 2 left; (-,-): 2 left; (+,-): 3 down -- each times sqrt 2
    assert np.allclose(d['road'][0], np.array([7.0, 2.0, 2.0, 3.0]) * math.sqrt(2), atol=1e-5)
    # the range is capped
    assert np.allclose(road_only((2.0, 3.0), exact_rays([(1, 0)]), max_range=5.0)['road'], 5.0)
    assert road_only((2.0, 3.0), exact_rays([(1, 0)]), max_range=5.0)['hit'][0, 0] == -1


def test_origin_off_the_road_gives_zero():
    out = road_only((-1.0, 5.0), exact_rays([(1, 0), (-1, 0), (0, 1)]))
    assert (out['road'] == 0.0).all() and (out['hit'] == -2).all()
    # within the tolerance of the edge the road is reached
    assert np.allclose(road_only((-0.01, 5.0), exact_rays([(1, 0)]))['road'], 10.01, atol=1e-6)


@pytest.mark.parametrize('gap, want', [(0.01, 15.01), (0.03, 5.0)])
def test_two_faces_separated_by_a_gap(gap, want):
    """two squares 10 m wide, the second one `gap` beyond the first: bridged below gap_tolerance = 0.02, the end of the road above"""
    x0 = np.float32(10.0) + np.float32(gap)
    verts = np.concatenate([SQUARE_V, np.array([[x0, 0], [x0 + 10, 0], [x0 + 10, 10], [x0, 10]], np.float32)])
    faces = np.concatenate([SQUARE_F, SQUARE_F + 4])
    out = road_only((5.0, 5.0), exact_rays([(1, 0)]), verts, faces)
    assert abs(out['road'][0, 0] - want) < 1e-5
    # zero-area and padding faces are no road: a degenerate face across the gap bridges nothing
    faces2 = np.concatenate([faces, [[0, 0, 0], [1, 4, 4]]])
    assert road_only((5.0, 5.0), exact_rays([(1, 0)]), verts, faces2, gap=0.0)['road'][0, 0] == 5.0


def two_boxes(ego_xy, others, ray_sc, present=None, max_range=50.0):
    boxes = np.array([[ego_xy[0], ego_xy[1], 4.0, 2.0, 0.0]] + others, np.float32)
    sc = np.stack([np.sin(boxes[:, 4]), np.cos(boxes[:, 4])], -1).astype(np.float32)
    present = [True] * len(boxes) if present is None else present
    return rm.range_scan(None, None, boxes, sc, present, ray_sc[None], max_range, 0.02)


def test_ray_parallel_to_a_box_side():
    other = [[10.0, 0.0, 4.0, 2.0, 0.0]]                       # x in [8, 12], y in [-1, 1]
    for y, want in ((0.5, 8.0), (1.0, 8.0), (-1.0, 8.0), (1.5, 50.0)):
        out = two_boxes((0.0, y), other, exact_rays([(1, 0)]))
        assert out['agents'][0, 0] == want and out['hit'][0, 0] == (1 if want < 50 else -1), (y, out)
    # ... and at an angle: from (0, 0) towards (8, 1), the near corner
    out = two_boxes((0.0, 0.0), other, rays([math.atan2(0.5, 8.0)]))
    assert abs(out['agents'][0, 0] - math.hypot(8.0, 0.5)) < 1e-5
    # a rotated box: the slab test runs in ITS frame
    out = two_boxes((0.0, 0.0), [[10.0, 0.0, 4.0, 2.0, math.pi / 2]], exact_rays([(1, 0)]))
    assert abs(out['agents'][0, 0] - 9.0) < 1e-5
    # behind the ray, absent, or the agent itself: nothing
    assert two_boxes((0.0, 0.0), other, exact_rays([(-1, 0)]))['agents'][0, 0] == 50.0
    assert two_boxes((0.0, 0.0), other, exact_rays([(1, 0)]), present=[True, False])['hit'][0, 0] == -1
    assert two_boxes((0.0, 0.0), other, exact_rays([(1, 0)]), max_range=8.0)['hit'][0, 0] == -1      # a hit AT max_range is none


def test_origin_inside_another_box_gives_zero():
    out = two_boxes((9.0, 0.5), [[10.0, 0.0, 4.0, 2.0, 0.3]], rays(np.linspace(-3, 3, 7)))
    assert (out['agents'] == 0.0).all() and (out['hit'] == 1).all()


def test_tie_goes_to_the_lowest_index():
    others = [[30.0, 0.0, 4.0, 2.0, 0.0], [10.0, 0.5, 4.0, 2.0, 0.0], [10.0, -0.5, 4.0, 2.0, 0.0]]
    out = two_boxes((0.0, 0.0), others, exact_rays([(1, 0)]))
    assert out['agents'][0, 0] == 8.0 and out['hit'][0, 0] == 2
    # the road decides where it ends first; an equal distance goes to the entity
    box = np.array([[2.0, 3.0, 4.0, 2.0, 0.0], [13.0, 3.0, 4.0, 2.0, 0.0], [8.0, 9.0, 4.0, 2.0, 0.0]], np.float32)
    sc = np.array([[0.0, 1.0]] * 3, np.float32)
    out = rm.range_scan(SQUARE_V, SQUARE_F, box, sc, [True] * 3, exact_rays([(1, 0), (0, 1), (-1, 0)])[None], 50.0, 0.02)
    assert list(out['hit'][0]) == [-2, -2, -2] and np.allclose(out['road'][0], [8.0, 7.0, 2.0])
    box[1, 0] = 12.0                                             # its near side at x = 10, where the road ends: 8 m both
    out = rm.range_scan(SQUARE_V, SQUARE_F, box, sc, [True] * 3, exact_rays([(1, 0)])[None], 50.0, 0.02)
    assert out['agents'][0, 0] == 8.0 and out['road'][0, 0] == 8.0 and out['hit'][0, 0] == 1
    # rows of absent exposed agents
    out = rm.range_scan(SQUARE_V, SQUARE_F, box, sc, [False, True, True], exact_rays([(1, 0)])[None], 50.0, 0.02)
    assert out['agents'][0, 0] == 50.0 and out['road'][0, 0] == 50.0 and out['hit'][0, 0] == -1


# ---- the table: float32 against float64 ---------------------------------------------------------------------------------------------------
TABLE_RAYS, TABLE_R, TABLE_RANGE = 9600, 64, 100.0
#: the GPU bar of tests/test_gpu_range_scan.py: 1e-4 m = 6 x 1.7e-5 m, the largest float32-against-float64 difference of the prototype of this
#: table; the table below must stay under 1e-4 / 6, or the bar is its own largest figure x 6
GPU_BAR = 1e-4


def town(name):
    t = np.load(os.path.join(GOLDEN, f'{name}_mesh.npz'))
    verts, faces, cats = t['verts'], t['faces'].astype(np.int64), [str(c) for c in t['categories']]
    road = t['vert_category'][faces[:, 0]] == cats.index('road')
    return verts, faces, road


def origins_on_road(verts, faces, n, seed):
    """n points inside road faces (area-weighted choice of the face, uniform inside it) and a heading each"""
    g = np.random.default_rng(seed)
    tri = verts[faces].astype(np.float64)
    area = np.abs((tri[:, 1, 0] - tri[:, 0, 0]) * (tri[:, 2, 1] - tri[:, 0, 1]) - (tri[:, 2, 0] - tri[:, 0, 0]) * (tri[:, 1, 1] - tri[:, 0, 1]))
    f = g.choice(len(faces), n, p=area / area.sum())
    u, v = g.random(n), g.random(n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    p = tri[f, 0] + u[:, None] * (tri[f, 1] - tri[f, 0]) + v[:, None] * (tri[f, 2] - tri[f, 0])
    return p.astype(np.float32), g.uniform(-np.pi, np.pi, n).astype(np.float32)


def table_rows():
    rows = []
    for name in ('town01', 'town02'):
        verts, faces, road = town(name)
        for what, sel in (('road faces', faces[road]), ('all faces', faces)):
            n = TABLE_RAYS // TABLE_R
            xy, psi = origins_on_road(verts, faces[road], n, seed=20251017)
            off = (-np.pi + 2 * np.pi * (np.arange(TABLE_R) + 0.5) / TABLE_R).astype(np.float32)
            ang = (psi[:, None] + off[None, :]).astype(np.float32)
            ray_sc = np.stack([np.sin(ang), np.cos(ang)], -1).astype(np.float32)
            r64 = np.stack([rm.road_ranges(verts, sel, xy[a], ray_sc[a][:, ::-1], TABLE_RANGE, 0.02, np.float64) for a in range(n)])
            r32 = np.stack([rm.road_ranges(verts, sel, xy[a], ray_sc[a][:, ::-1], TABLE_RANGE, 0.02, np.float32) for a in range(n)])
            diff = np.abs(r32.astype(np.float64) - r64)
            rows.append(dict(map=name, faces=what, rays=diff.size, max_diff=float(diff.max()), beyond_1e_4=int((diff > 1e-4).sum()),
                             mean_range=float(r64.mean()), at_zero=int((r64 == 0).sum()), at_max=int((r64 == TABLE_RANGE).sum())))
    return rows


def test_float32_against_float64_table():
    """Measured here (seed 20251017, 4 x 9 600 rays, max_range 100 m, gap_tolerance 0.02 m): see the printed table; the assertion is the one the
    GPU bar rests on -- the largest difference x 6 stays within GPU_BAR, and no ray is beyond it."""
    rows = table_rows()
    print()
    print(f'{"map":8s} {"faces":11s} {"rays":>6s} {"max |f32 - f64| m":>18s} {"> 1e-4 m":>9s} {"mean range m":>13s} {"at 0":>6s} {"at max":>7s}')
    for r in rows:
        print(f'{r["map"]:8s} {r["faces"]:11s} {r["rays"]:6d} {r["max_diff"]:18.3e} {r["beyond_1e_4"]:9d} {r["mean_range"]:13.2f} {r["at_zero"]:6d} {r["at_max"]:7d}')
    assert all(r['rays'] >= 9600 for r in rows)
    # origins inside road faces: no ray starts off the road
    assert all(r['at_zero'] == 0 for r in rows)
    worst = max(r['max_diff'] for r in rows)
    assert worst * 6 <= GPU_BAR, f'the largest float32-against-float64 difference is {worst:.3e} m: the GPU bar would have to be {6 * worst:.3e} m'
    assert sum(r['beyond_1e_4'] for r in rows) == 0
