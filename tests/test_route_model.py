"""The float64 model of route goals (tests/route_model.py) against what it has to get right on its own: routes that follow the
lane graph and have the length that was asked for, points and progress that invert each other, progress that stays monotone where a route laps a
ring, rows that get no route.  Maps: a hand-built ring of four 20 m lanelets with a fork, the three unconnected lanelets of
testing_lanelet2map.osm, Town01 and Town02.  No GPU."""
import math
import os

import numpy as np
import pytest

import lane_follow_model as lf
import route_model as rm
from conftest import GOLDEN


@pytest.fixture(scope='module')
def lanes():
    from torchdrivesim_amd import lanelet2
    out = {k: rm.Lanes(lanelet2.load_lanelet_map(os.path.join(GOLDEN, f), origin=(0.0, 0.0)))
           for k, f in (('Town01', 'carla_Town01.osm.gz'), ('Town02', 'carla_Town02.osm.gz'), ('testing', 'testing_lanelet2map.osm'))}
    out['ring'] = rm.Lanes(rm.ring_with_fork())
    return out


def random_starts(model, count, g):
    ok = [l for l in range(len(model)) if model.eligible(l) and not model.flag[l]]
    return [(int(l), float(g.uniform(0.0, 1.0)) * model.length(int(l))) for l in g.choice(ok, count)]


def lap_route(model, laps_length=200.0, start=(0, 2.5)):
    """a route on the ring that never takes the fork's dead end: the first (seed, agent) whose draws stay on the ring"""
    for seed in range(4000):
        r = rm.sample(model, start[0], start[1], laps_length, seed, 0, 0)
        if r.length == laps_length:
            return r, seed
    raise AssertionError('no seed keeps a 200 m route on the ring')


def test_the_route_stream_is_its_own():
    """same seed, scene, row and hop: a word of its own, neither the NPCs' nor spawn's"""
    words = {rm.route_word(7, 3, 2, 1), lf.route_word(7, 3, 2, 1), lf.philox4x32_10((3, 0, 2, 1), (7, 0))[0]}
    assert len(words) == 3
    assert rm.route_word(2 ** 64 + 7, 3, 2, 1) == rm.route_word(7, 3, 2, 1)


def test_the_ring_is_what_the_tests_take_it_for(lanes):
    ring = lanes['ring']
    assert ring.succ == [[1, 4], [2], [3], [0], []]
    assert [ring.length(l) for l in range(5)] == [20.0] * 5 and all(len(c) == 5 for c in ring.cl)


@pytest.mark.parametrize('name', ['ring', 'testing', 'Town01', 'Town02'])
def test_routes_follow_the_graph_and_have_the_length_asked_for(lanes, name):
    model = lanes[name]
    g = np.random.default_rng(11)
    count = 4000 if name.startswith('Town') else 400
    short = hops = pts = 0
    for row, (l, arc) in enumerate(random_starts(model, count, g)):
        D = 200.0 if name.startswith('Town') else float(g.uniform(1.0, 250.0))
        r = rm.sample(model, l, arc, D, seed=5, scene_id=row // 8, agent=row % 8)
        assert r.n >= 1 and r.lanes[0] == l and r.start_arc == arc
        for a, b in zip(r.lanes, r.lanes[1:]):
            assert b in model.succ[a], 'consecutive route lanelets are graph edges'
        total = 0.0
        for j in range(r.n):
            assert r.offsets[j] == total
            a, b = r.interval(model, j)
            assert 0.0 <= a <= b <= model.length(r.lanes[j])
            total = total + (b - a)
        assert r.length == total
        last = r.lanes[-1]
        if abs(r.length - D) > 1e-9:
            # short: the route stands at the end of a dead end (nothing follows, or the drawn successor cannot be driven) or of its 16th lanelet
            assert r.length < D and r.end_arc == model.length(last)
            assert r.n == rm.MAX_LANES or rm.successor(model, last, 5, row // 8, row % 8, r.n - 1) < 0
            short += 1
        else:
            assert r.end_arc <= model.length(last)
        hops, pts = max(hops, r.n - 1), max(pts, sum(len(model.cl[x]) for x in r.lanes))
    print(name, 'short routes', short, 'of', count, 'most hops', hops, 'most centre-line points', pts)
    if name.startswith('Town'):
        # the shipped towns have no dead end and 200 m never needs the 16-lanelet cap
        assert short == 0 and hops <= 9
    if name == 'testing':
        assert hops == 0, 'three lanelets without successors: every route ends on its own lanelet'
    if name == 'ring':
        assert 0 < short < count


def test_every_route_of_the_small_map_is_a_dead_end(lanes):
    model = lanes['testing']
    for l in range(3):
        r = rm.sample(model, l, 1.0, 1000.0, 1, 0, l)
        assert r.lanes == [l] and r.end_arc == model.length(l) and r.length == model.length(l) - 1.0
        assert rm.sample(model, l, model.length(l), 10.0, 1, 0, l).n == 0, 'a start at the very end of a dead end is no route'


def test_the_cap_ends_a_route_at_its_sixteenth_lanelet(lanes):
    ring = lanes['ring']
    for seed in range(20000):
        r = rm.sample(ring, 1, 0.0, 1000.0, seed, 0, 0)
        if r.n == rm.MAX_LANES:
            break
    assert r.n == 16 and r.length == 320.0 and r.end_arc == 20.0 and r.lanes[:5] == [1, 2, 3, 0, 1]


def test_rows_that_get_no_route(lanes):
    ring = lanes['ring']
    assert rm.sample(ring, 0, 1.0, 50.0, 1, 0, 0).n >= 2
    for kw in (dict(lane=-1), dict(lane=99), dict(distance=float('nan')), dict(distance=float('inf')), dict(distance=0.0), dict(distance=-3.0),
               dict(present=False)):
        args = dict(lane=0, arc=1.0, distance=50.0, seed=1, scene_id=0, agent=0)
        args.update(kw)
        r = rm.sample(ring, **args)
        assert r.n == 0 and r.length == 0.0, kw
        out = rm.progress(ring, r, 1.0, 0.0, 0.0, 1.0, K=3)
        assert not out['found'] and out['heading'].tolist() == [0.0, 1.0] and not out['lookahead'].any() and out['progress'] == 0
        assert rm.points(ring, r, [0.0, 5.0]).tolist() == [[0.0, 0.0]] * 2
    assert rm.sample(None, 0, 1.0, 50.0, 1, 0, 0).n == 0


@pytest.mark.parametrize('name', ['ring', 'testing', 'Town01', 'Town02'])
def test_progress_inverts_points(lanes, name):
    """progress(points(q)) == q to 1e-9, the cursor on q's piece, lateral and heading error 0, walking each route front to back in steps of 3 m
    (a step at 30 m/s) -- lookahead point m is the point at q + (m + 1) * spacing seen from there"""
    model = lanes[name]
    g = np.random.default_rng(5)
    worst = 0.0
    for row, (l, arc) in enumerate(random_starts(model, 12, g)):
        r = rm.sample(model, l, arc, 200.0, seed=9, scene_id=0, agent=row)
        if r.n == 0:
            continue
        first = True
        for q in list(np.arange(0.0, r.length, 3.0)) + [r.length]:
            x, y = rm.point(model, r, q)
            out = rm.progress(model, r, x, y, 0.0, 1.0, K=4, spacing=2.5, exact=True)
            worst = max(worst, abs(out['progress'] - q))
            assert abs(out['progress'] - q) <= 1e-9, (name, row, q, out['progress'])
            j = out['piece']
            assert r.cursor == j and (r.offsets[j] - 1e-9 <= q) and (q <= (r.offsets[j + 1] if j + 1 < r.n else r.length) + 1e-9)
            assert abs(out['lateral']) <= 1e-9 and out['remaining'] == r.length - out['progress']
            assert out['advance'] == out['progress'] - (0.0 if first else previous)
            assert out['reached'] == (out['remaining'] <= 2.0) and r.completed == (out['remaining'] <= 2.0) and not out['off_route']
            # heading [0, 1] is psi = 0: the error's [sin, cos] is then [-t.y, t.x]
            assert abs(math.hypot(*out['heading']) - 1.0) <= 1e-12
            for m in range(4):
                px, py = rm.point(model, r, out['progress'] + (m + 1) * 2.5)
                assert out['lookahead'][m].tolist() == [(px - x) * 1.0 + (py - y) * 0.0, (py - y) * 1.0 - (px - x) * 0.0]
            previous, first = out['progress'], False
    print(name, 'worst |progress(points(q)) - q|', worst)


def test_progress_is_monotone_round_the_ring_twice(lanes):
    """a 200 m route on an 80 m ring: two and a half laps.  Every pose lies on two or three pieces of the route; the cursor's window of three
    pieces keeps each on its own lap."""
    ring = lanes['ring']
    r, _ = lap_route(ring)
    assert r.n == 11 and r.lanes == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2]
    g = np.random.default_rng(2)
    last, seen = -1.0, []
    for q in np.arange(0.0, 200.0, 1.7):
        x, y = rm.point(ring, r, q)
        x, y = x + float(g.uniform(-0.4, 0.4)), y + float(g.uniform(-0.4, 0.4))            # beside the centre line, as a car is
        out = rm.progress(ring, r, rm.F32(x), rm.F32(y), 0.0, 1.0, exact=True)
        assert out['progress'] >= last - 0.9 and abs(out['progress'] - q) < 0.9, (q, out['progress'], last)
        assert r.cursor >= (seen[-1] if seen else 0)
        last = max(last, out['progress'])
        seen.append(r.cursor)
    assert seen[-1] == 10 and sorted(set(seen)) == list(range(11)) and r.completed


def test_the_window_keeps_a_pose_on_its_lap(lanes):
    """the same pose, 7.5 m along lanelet 1, is on pieces 1, 5 and 9 of the lapping route: the cursor decides which, and the earliest wins inside
    one window"""
    ring = lanes['ring']
    r, _ = lap_route(ring)
    x, y = rm.point(ring, r, 25.0)
    for cursor, want in ((0, 25.0), (1, 25.0), (3, 105.0), (4, 105.0), (5, 105.0), (7, 185.0), (8, 185.0), (9, 185.0)):
        r.cursor = cursor
        out = rm.progress(ring, r, x, y, 1.0, 0.0, exact=True)
        assert abs(out['progress'] - want) < 1e-9 and r.cursor == {25.0: 1, 105.0: 5, 185.0: 9}[want], (cursor, out['progress'])
    # a window that holds no piece on that lanelet (cursor 2: lanelets 2, 3, 0) finds the nearest point of what it does hold, never an earlier lap
    r.cursor = 2
    out = rm.progress(ring, r, x, y, 1.0, 0.0, exact=True)
    assert r.cursor == 4 and out['progress'] == 97.5, 'the end of lanelet 0 on its second lap'


def test_ties_go_to_the_earliest_segment(lanes):
    """a corner of the ring is the end of one lanelet and the start of the next: a pose on the diagonal through it is equally far from both and
    belongs to the earlier"""
    ring = lanes['ring']
    r, _ = lap_route(ring)
    out = rm.progress(ring, r, 21.0, -1.0, 0.0, 1.0, exact=True)                 # outside corner 1, on the diagonal
    assert (out['piece'], out['segment']) == (0, 3) and out['progress'] == 17.5
    assert out['lateral'] == -1.0 and out['heading'].tolist() == [0.0, 1.0]
    out = rm.progress(ring, r, 10.0, 6.0, 1.0, 0.0, exact=True)
    assert out['off_route'] and out['lateral'] == 6.0 and out['heading'].tolist() == [1.0, 0.0], 'left of the lane, heading 90 degrees off it'


def test_a_route_inside_one_lanelet_and_one_of_a_single_segment(lanes):
    ring = lanes['ring']
    r = rm.sample(ring, 2, 6.0, 3.0, 1, 0, 0)                                    # ends inside its first lanelet, and inside one segment
    assert r.lanes == [2] and (r.start_arc, r.end_arc, r.length) == (6.0, 9.0, 3.0)
    for x, want in ((25.0, 0.0), (13.0, 1.0), (0.0, 3.0)):                        # lanelet 2 runs from (20, 20) to (0, 20): clipped to its 3 m
        out = rm.progress(ring, r, x, 20.0, 0.0, -1.0, exact=True)
        assert out['progress'] == want and out['segment'] == 1
    assert out['reached'] and r.completed
    assert rm.point(ring, r, 99.0) == (11.0, 20.0) and rm.point(ring, r, -1.0) == (14.0, 20.0)
