"""The float64 autograd model of the differentiable route step (tests/route_grad_model.py) against the model of the forward it
differentiates (tests/route_model.py): its forward equals route_model.progress(exact=True) bit for bit, and its gradients equal central
differences of route_model.progress(exact=True).

Central differences: step h = 1e-5 in each of x, y, sin, cos, on poses at least 1e-3 m from every kink (the discrete choices -- piece, segment,
active clamp, the lookahead's pieces, segments and clamps -- are the same on the eight poses 1e-3 m around), within 1e-6: inside such a cell every
output is linear or bilinear in the inputs, so a central difference has no truncation error and only rounding is left, about
2e-16 x 1e3 (the largest coordinate) / 1e-5 = 2e-8.  Maps: the ring of route_model.ring_with_fork, and Town01.  No GPU."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import route_grad_model as rgm
import route_model as rm
from conftest import GOLDEN

H, NEAR, TOL = 1e-5, 1e-3, 1e-6
F32 = np.float32


@pytest.fixture(scope='module')
def lanes():
    from torchdrivesim_amd import lanelet2
    return {'ring': rm.Lanes(rm.ring_with_fork()),
            'Town01': rm.Lanes(lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'carla_Town01.osm.gz'), origin=(0.0, 0.0)))}


def flat(out, K):
    """the float outputs of a progress call as one vector: progress, advance, remaining, lateral, heading (2), lookahead (2 K)"""
    return np.concatenate([[out['progress'], out['advance'], out['remaining'], out['lateral']], np.asarray(out['heading'], np.float64),
                           np.asarray(out['lookahead'], np.float64).reshape(-1)])


def at_cursor(route, q):
    """a copy of the route whose cursor stands on the piece that holds route arc q, and whose stored progress is not zero"""
    r = copy.copy(route)
    r.cursor = max([j for j in range(route.n) if route.offsets[j] <= q] or [0])
    r.stored = 0.75 * q
    return r


def pose_near(model, route, q, left=0.0, turn=0.0, along=0.0):
    """[x, y, sin, cos] as float32 values: `left` metres beside the route at arc q, `along` metres further in its direction (beyond an end where q
    is one), heading `turn` off it"""
    x, y = rm.point(model, route, q)
    back = q + 0.25 > route.length
    x2, y2 = rm.point(model, route, q - 0.25 if back else q + 0.25)
    tx, ty = ((x - x2), (y - y2)) if back else ((x2 - x), (y2 - y))
    n = math.hypot(tx, ty)
    tx, ty = tx / n, ty / n
    psi = math.atan2(ty, tx) + turn
    return [float(F32(x - left * ty + along * tx)), float(F32(y + left * tx + along * ty)), float(F32(math.sin(psi))), float(F32(math.cos(psi)))]


def signature(model, route, pose, K, spacing):
    ch = rgm.choices(model, route, *pose, K=K, spacing=spacing)
    return None if ch is None else (ch['piece'], ch['segment'], ch['clamp'], tuple(ch['look']))


def settled(model, route, pose, K, spacing):
    """no kink within NEAR of the pose: the same discrete choices on the eight poses around it"""
    want = signature(model, route, pose, K, spacing)
    ring = [(NEAR * math.cos(t), NEAR * math.sin(t)) for t in np.arange(8) * (math.pi / 4)]
    return want is not None and all(signature(model, route, [pose[0] + ex, pose[1] + ey] + pose[2:], K, spacing) == want for ex, ey in ring)


def jacobian(model, route, pose, K, spacing):
    """(outputs, 4) from the autograd model, and its forward as a vector"""
    xy, sc, out = rgm.forward(model, route, pose[:2], pose[2:], K, spacing)
    vec = torch.cat([torch.stack([out['progress'], out['advance'], out['remaining'], out['lateral']]), out['heading'], out['lookahead'].reshape(-1)])
    rows = []
    for v in vec:
        g = torch.autograd.grad(v, (xy, sc), retain_graph=True, allow_unused=True)
        rows.append(np.concatenate([np.zeros(2) if t is None else t.numpy() for t in g]))
    return np.array(rows), vec.detach().numpy()


def differences(model, route, pose, K, spacing):
    cols = []
    for c in range(4):
        side = []
        for s in (1.0, -1.0):
            p = list(pose)
            p[c] = p[c] + s * H
            side.append(flat(rm.progress(model, copy.copy(route), *p, K=K, spacing=spacing, exact=True), K))
        cols.append((side[0] - side[1]) / (2.0 * H))
    return np.array(cols).T


def hold(model, route, pose, K, spacing, what):
    """-> the model's Jacobian, after holding its forward to route_model bit for bit and itself to central differences"""
    assert settled(model, route, pose, K, spacing), (what, 'the test put this pose on a kink')
    jac, vec = jacobian(model, route, pose, K, spacing)
    ref = flat(rm.progress(model, copy.copy(route), *pose, K=K, spacing=spacing, exact=True), K)
    assert vec.tobytes() == ref.tobytes(), (what, vec, ref)
    cd = differences(model, route, pose, K, spacing)
    worst = float(np.abs(jac - cd).max())
    assert worst <= TOL, (what, worst, jac, cd)
    return jac, worst


def ring_route(model, length=200.0, start=(0, 2.5)):
    for seed in range(4000):
        r = rm.sample(model, start[0], start[1], length, seed, 0, 0)
        if r.length == length:
            return r
    raise AssertionError('no seed keeps the route on the ring')


def test_interior_feet_on_the_ring(lanes):
    ring = lanes['ring']
    route = ring_route(ring)
    worst, done = 0.0, 0
    for n, q in enumerate(np.arange(1.3, 160.0, 7.9)):
        pose = pose_near(ring, route, q, left=0.7 * math.sin(n), turn=0.3 * math.cos(n))
        r = at_cursor(route, q)
        if not settled(ring, r, pose, 5, 3.0):
            continue
        jac, w = hold(ring, r, pose, 5, 3.0, ('ring', q))
        worst, done = max(worst, w), done + 1
        assert abs(np.hypot(*jac[0, :2]) - 1.0) < 1e-9, 'an interior foot moves along its segment at unit rate on a flat centre line'
        assert np.array_equal(jac[1], jac[0]) and np.array_equal(jac[2], -jac[0]), 'advance as progress, remaining as its negative'
        assert not jac[:4, 2:].any() and not jac[4:6, :2].any(), 'the scalars do not see the heading, the heading error does not see the position'
    print('ring, interior feet:', done, 'poses, worst |autograd - central difference|', worst)
    assert done >= 12


def test_interior_feet_on_town01(lanes):
    town = lanes['Town01']
    g = np.random.default_rng(3)
    ok = [l for l in range(len(town)) if town.eligible(l) and not town.flag[l]]
    worst, done, pieces = 0.0, 0, set()
    for row, l in enumerate(g.choice(ok, 10)):
        route = rm.sample(town, int(l), 0.3 * town.length(int(l)), 200.0, seed=13, scene_id=0, agent=row)
        assert route.n >= 1
        for q in g.uniform(0.5, route.length - 0.5, 6):
            pose = pose_near(town, route, float(q), left=float(g.uniform(-0.8, 0.8)), turn=float(g.uniform(-0.4, 0.4)))
            r = at_cursor(route, float(q))
            if not settled(town, r, pose, 8, 4.0):
                continue
            _, w = hold(town, r, pose, 8, 4.0, ('Town01', row, q))
            worst, done = max(worst, w), done + 1
            pieces.add((row, rgm.choices(town, r, *pose, K=8, spacing=4.0)['piece']))
    print('Town01, interior feet:', done, 'poses on', len(pieces), 'pieces, worst |autograd - central difference|', worst)
    assert done >= 30 and len(pieces) >= 15


def test_feet_clamped_at_the_start_and_at_the_end(lanes):
    """a pose behind the route's start, and one beyond its end (a route that ends inside a segment): the foot stands still, so progress, advance
    and remaining have no gradient; lateral and heading keep theirs, and the lookahead keeps its direct part"""
    ring = lanes['ring']
    route = rm.sample(ring, 0, 2.5, 6.0, 1, 0, 0)                           # from 2.5 to 8.5 on lanelet 0: two segments, both ends inside one
    assert route.lanes == [0] and (route.start_arc, route.end_arc) == (2.5, 8.5)
    for along, q, clamp in ((-1.5, 0.0, -1), (1.25, route.length, 1)):
        pose = pose_near(ring, route, q, left=0.4, turn=0.2, along=along)
        ch = rgm.choices(ring, route, *pose, K=3, spacing=1.0)
        assert ch['clamp'] == clamp and ch['out']['progress'] == q
        jac, _ = hold(ring, route, pose, 3, 1.0, ('clamped', clamp))
        assert not jac[:3].any(), 'a clamped foot does not move'
        assert jac[3, :2].tolist() == [0.0, 1.0] and jac[4:6, 2:].any(), 'lateral against the line of the segment, clamped or not'
        assert np.array_equal(jac[6::2, :2], np.tile([-pose[3], -pose[2]], (3, 1))), 'd ox / d[x, y] = -[cos, sin]: the direct part alone'
    # equality counts as interior: a pose exactly over the start of the route (u_raw == ulo, representable: x = 2.5 on a segment from 0 to 5)
    xy, sc, out = rgm.forward(ring, route, [2.5, 0.25], [0.0, 1.0], K=0)
    g, = torch.autograd.grad(out['progress'], xy)
    assert float(out['progress'].detach()) == 0.0 and g.tolist() == [1.0, 0.0]


def test_lookahead_beyond_the_end_has_no_gradient_through_progress(lanes):
    ring = lanes['ring']
    route = rm.sample(ring, 0, 2.5, 12.0, 1, 0, 0)
    assert route.lanes == [0] and route.length == 12.0
    pose = pose_near(ring, route, 7.1, left=-0.3, turn=0.1)
    ch = rgm.choices(ring, route, *pose, K=4, spacing=2.0)
    assert [m for _, _, m in ch['look']] == [True, True, False, False], 'points at 9.1 and 11.1 of 12 m, then two beyond the end'
    jac, _ = hold(ring, route, pose, 4, 2.0, 'beyond the end')
    sn, cs = pose[2], pose[3]
    for m in range(4):
        ox = jac[6 + 2 * m, :2]
        direct = np.array([-cs, -sn])
        if m < 2:                                                           # the point moves with the foot: d ox / dx = -cs + (Q.x cs + Q.y sn) D.x, Q = D = [1, 0]
            assert np.allclose(ox, direct + np.array([cs, 0.0]), atol=1e-12)
        else:
            assert np.array_equal(ox, direct), 'a point held at the end moves with nothing but the agent'
    assert np.array_equal(jac[6 + 4:6 + 6, 2:], jac[6 + 6:, 2:]), 'both are the same point, the route\'s end'


def test_no_lookahead_absent_rows_and_rows_without_a_route(lanes):
    ring = lanes['ring']
    route = ring_route(ring)
    pose = pose_near(ring, route, 33.3, left=0.5, turn=-0.2)
    r = at_cursor(route, 33.3)
    jac, _ = hold(ring, r, pose, 0, 4.0, 'K = 0')
    assert jac.shape == (6, 4)
    every = dict(progress=1.0, advance=-2.0, lateral=0.5, heading=[0.3, -0.7], remaining=4.0, lookahead=np.ones((0, 2)))
    g_xy, g_sc = rgm.gradients(ring, r, pose[:2], pose[2:], every, K=0)
    assert np.allclose(g_xy, (1.0 - 2.0 - 4.0) * jac[0, :2] + 0.5 * jac[3, :2], atol=1e-15) and np.allclose(g_sc, 0.3 * jac[4, 2:] - 0.7 * jac[5, 2:], atol=1e-15)
    assert not np.array_equal(g_xy, np.zeros(2)) and not np.array_equal(g_sc, np.zeros(2))
    every['lookahead'] = np.ones((3, 2))
    for what, kw in (('absent', dict(route=r, present=False)), ('no route', dict(route=rm.Route())), ('no table', dict(route=r, lanes=None)),
                     ('NaN pose', dict(route=r, xy=[float('nan'), pose[1]]))):
        args = dict(lanes=ring, xy=pose[:2], sc=pose[2:], grads=every, K=3, spacing=4.0)
        args.update(kw)
        for dtype in (torch.float64, torch.float32):
            g_xy, g_sc = rgm.gradients(dtype=dtype, **args)
            assert not g_xy.any() and not g_sc.any(), what
        assert rgm.forward(args['lanes'], args['route'], args['xy'], args['sc'], 3, 4.0, args.get('present', True))[2] is None, what


def test_the_float32_yardstick_makes_the_same_choices(lanes):
    """dtype=float32: the float64 choices with float32 arithmetic -- close to the float64 gradients, and not equal to them"""
    town = lanes['Town01']
    l = max(range(len(town)), key=lambda l: town.length(l) if town.eligible(l) and not town.flag[l] else 0.0)
    route = rm.sample(town, l, 3.0, 200.0, seed=2, scene_id=0, agent=0)
    g = np.random.default_rng(8)
    grads = dict(progress=0.7, advance=-0.2, lateral=1.1, heading=g.normal(size=2), remaining=0.4, lookahead=g.normal(size=(16, 2)))
    pose = pose_near(town, route, 41.7, left=0.6, turn=0.25)
    r = at_cursor(route, 41.7)
    g64 = np.concatenate(rgm.gradients(town, r, pose[:2], pose[2:], grads))
    g32 = np.concatenate(rgm.gradients(town, r, pose[:2], pose[2:], grads, dtype=torch.float32))
    err = float(np.abs(g64 - g32).max())
    print('float32 yardstick against float64:', err, 'of', float(np.abs(g64).max()))
    assert 0.0 < err <= 1e-3 * float(np.abs(g64).max())
