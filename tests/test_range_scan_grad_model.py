"""
The float64 autograd model of the range-scan backward (tests/range_scan_grad_model.py: scene_gradients' ranges_given_choices, with the MODEL's own
choices) against central differences of the restated forward (forward64), and closed-form cases.  CPU only.

Step h = 1e-5 in x, y and psi of the observer and in x, y, psi, length and width of the entity a ray ends on; bar 1e-6 x (1 + |gradient|), the
siblings' figure.  A probe (ray, parameter) is left out only where the model's choice -- entity, slab, exit edge, the chain of the fixed point (the
gaps it bridged) -- differs between the two probe points; at most 1 % of the live probes may be, which is asserted from the model alone before anything is
compared.
"""
import numpy as np
import pytest
import torch

import range_scan_grad_model as gm
from test_range_scan_model import origins_on_road, town

H = 1e-5
BAR = 1e-6
CAP = 0.01
PARAMS = ('x', 'y', 'length', 'width', 'psi')


def offsets(R, fov=2 * np.pi):
    k = np.arange(R, dtype=np.float64)
    return -fov / 2 + (fov * (k + 0.5)) / R


def scene_of(boxes, A, R):
    """float64 boxes (E, 5) -> sc (E, 2), ray_sc (A, R, 2): [sin, cos] of psi and of psi + off_k, in float64"""
    ang = boxes[:A, 4, None] + offsets(R)
    return np.stack([np.sin(boxes[:, 4]), np.cos(boxes[:, 4])], -1), np.stack([np.sin(ang), np.cos(ang)], -1)


def forward(tri, boxes, present, A, R, max_range, gap=0.02):
    sc, ray_sc = scene_of(boxes, A, R)
    return gm.forward64(tri, boxes, sc, present, ray_sc, max_range, gap)


def model_jvp(boxes, A, R, choice, edges, entity, col):
    """d (t_agent, t_road) / d boxes[entity, col] for every ray, by forward-mode differentiation of the autograd model given the choices; psi
    reaches the ranges through [sin, cos] of the entity and of its rays"""
    off = torch.from_numpy(offsets(R))
    ch, ed = torch.from_numpy(choice)[None], torch.from_numpy(edges)[None]

    def fn(b):
        sc = torch.stack([torch.sin(b[:, 4]), torch.cos(b[:, 4])], -1)
        ang = b[:A, 4, None] + off
        ray_sc = torch.stack([torch.sin(ang), torch.cos(ang)], -1)
        ta, _, tr, _ = gm.ranges_given_choices(b[None], sc[None], ray_sc[None], ch, ed)
        return ta[0], tr[0]
    v = torch.zeros(boxes.shape, dtype=torch.float64)
    v[entity, col] = 1.0
    _, (da, dr) = torch.autograd.functional.jvp(fn, torch.from_numpy(boxes), v)
    return da.numpy(), dr.numpy()


def probe_scene(tri, boxes, present, A, R, max_range, probes):
    """-> list of (what, |model - difference|, |model|, live, same): one entry per (probe, part), arrays over the scene's A x R rays"""
    centre = forward(tri, boxes, present, A, R, max_range)
    edges = gm.edges_array(centre['edge'], A, R)
    live_a = (centre['choice'][..., 0] >= 0) & (centre['choice'][..., 1] > 0)
    live_r = np.isfinite(edges).all(-1)
    out = []
    for entity, col in probes:
        lo, hi = boxes.copy(), boxes.copy()
        lo[entity, col] -= H
        hi[entity, col] += H
        f_lo, f_hi = forward(tri, lo, present, A, R, max_range), forward(tri, hi, present, A, R, max_range)
        da, dr = model_jvp(boxes, A, R, centre['choice'], edges, entity, col)
        same_a = (f_lo['choice'] == centre['choice']).all(-1) & (f_hi['choice'] == centre['choice']).all(-1)
        same_r = np.array([[f_lo['edge'][a][k] == centre['edge'][a][k] == f_hi['edge'][a][k] and
                            f_lo['chain'][a][k] == centre['chain'][a][k] == f_hi['chain'][a][k] for k in range(R)] for a in range(A)])
        # a probe that does not reach the ray (another entity's pose) is live only if the model says the ray depends on it
        dep_a = live_a & ((centre['choice'][..., 0] == entity) | (np.arange(A)[:, None] == entity))
        dep_r = live_r & (np.arange(A)[:, None] == entity)
        out.append((f'agents d/d {PARAMS[col]} of {entity}', np.abs(da - (f_hi['agents'] - f_lo['agents']) / (2 * H)), np.abs(da), dep_a, same_a))
        out.append((f'road d/d {PARAMS[col]} of {entity}', np.abs(dr - (f_hi['road'] - f_lo['road']) / (2 * H)), np.abs(dr), dep_r, same_r))
        assert not da[~dep_a].any() and not dr[~dep_r].any(), 'the model gives a ray no gradient to something it does not depend on'
    return out


def judge(label, rows, least):
    live = sum(int(r[3].sum()) for r in rows)
    left_out = sum(int((r[3] & ~r[4]).sum()) for r in rows)
    print(f'{label}: {live} live probes, {left_out} left out (the model\'s choice differs between the probe points)')
    assert live >= least and left_out <= CAP * live, (label, live, left_out)
    worst = 0.0
    for what, diff, mag, dep, same in rows:
        keep = dep & same
        if keep.any():
            rel = diff[keep] / (1 + mag[keep])
            worst = max(worst, float(rel.max()))
            assert (rel <= BAR).all(), f'{label} {what}: {float(rel.max()):.3g} beyond {BAR}'
    print(f'{label}: largest |model - central difference| / (1 + |gradient|) = {worst:.3g}')


def test_town01_road_rays_against_central_differences():
    """40 origins inside road faces, 64 rays, 50 m: x, y, psi of the observer"""
    verts, faces, road = town('town01')
    xy, psi = origins_on_road(verts, faces[road], 40, seed=20251021)
    rows, reach = [], 51.0
    for o, p in zip(xy.astype(np.float64), psi.astype(np.float64)):
        tri = gm.near_faces(verts, faces, o, reach)
        boxes = np.array([[o[0], o[1], 4.5, 2.0, p]])
        rows += probe_scene(tri, boxes, np.ones(1, bool), 1, 64, 50.0, [(0, 0), (0, 1), (0, 4)])
    judge('town01', rows, least=3000)


def test_rectangles_against_central_differences():
    """3 scenes of 12 random rectangles, 4 observers of 16 rays: x, y, psi, length and width of every entity"""
    rows = []
    for seed in (11, 12, 13):
        s = gm.random_boxes(seed, 1, 4, 12, spread=14.0)
        boxes, present = s['boxes'][0].astype(np.float64), s['present'][0]
        rows += probe_scene(None, boxes, present, 4, 16, 50.0, [(e, c) for e in range(12) for c in range(5)])
    judge('rectangles', rows, least=300)


def test_a_ray_square_on_a_box_face():
    """d t / d x_obs = -1 and d t / d length = -1/2, and the entity's x gets +1"""
    boxes = np.array([[[0.0, 0.0, 4.0, 2.0, 0.0], [10.0, 0.3, 4.0, 2.0, 0.0]]])
    sc = np.array([[[0.0, 1.0], [0.0, 1.0]]])
    ray_sc = np.array([[[[0.0, 1.0]]]])
    t0, j, slab = gm.agent_choice(boxes[0], sc[0], np.ones(2, bool), 0, (1.0, 0.0))
    assert (t0, j, slab) == (8.0, 1, 1)
    gb, gsc, gr, la, _ = gm.scene_gradients(boxes, sc, ray_sc, np.array([[[[j, slab]]]]), np.full((1, 1, 1, 4), np.nan), np.ones((1, 1, 1)), None)
    assert la.all() and gb[0, 0].tolist() == [-1.0, 0.0, 0.0, 0.0, 0.0] and gb[0, 1].tolist() == [1.0, 0.0, -0.5, 0.0, 0.0]
    # t = (-h - rx c) / (dx c): d t / d cos = -rx / e - t dx / e = 10 - 8, d t / d sin = -ry / e, d t / d dx = -t / e
    assert gsc[0, 1, 1] == pytest.approx(2.0) and gsc[0, 1, 0] == pytest.approx(0.3) and gr[0, 0, 0, 1] == pytest.approx(-8.0)


@pytest.mark.parametrize('alpha', [np.pi / 2, np.pi / 3, 0.2])
def test_a_ray_meeting_a_straight_road_edge(alpha):
    """|grad_o t| = 1 / sin(alpha), directed along the edge's normal (towards the edge the range shrinks)"""
    edge = np.array([[[[-50.0, 7.0, 80.0, 7.0]]]])                                  # the line y = 7, the observer below it
    boxes = np.array([[[1.0, 2.0, 4.0, 2.0, 0.0]]])
    ray_sc = np.array([[[[np.sin(alpha), np.cos(alpha)]]]])
    gb, _, _, _, lr = gm.scene_gradients(boxes, np.array([[[0.0, 1.0]]]), ray_sc, np.array([[[[-1, 0]]]]), edge, None, np.ones((1, 1, 1)))
    assert lr.all() and gb[0, 0, 0] == pytest.approx(0.0, abs=1e-12) and gb[0, 0, 1] == pytest.approx(-1 / np.sin(alpha), rel=1e-12)


def test_the_models_own_edge_rule_on_a_square():
    """a unit-speed ray from inside a square of two triangles leaves through the side it points at; the diagonal, which both faces share and the
    ray crosses first, is not the exit"""
    tri = np.array([[[0, 0], [10, 0], [10, 10]], [[0, 0], [10, 10], [0, 10]]], np.float64)
    (F, edge, chain), = gm.road_choice(tri, (2.0, 1.0), np.array([[0.0, 1.0]]), 50.0, 0.02)
    assert F == 9.0 and edge == (0.0, 10.0, 10.0, 10.0) and chain == ()
