"""The float64 model of lane-following NPC traffic (tests/lane_follow_model.py) against what it has to get right on its own -- the lane graph of
the shipped maps, poses recovered from centre lines, the IDM's closed forms, a queue that comes to rest, hops that keep the distance, dead
ends, the route stream -- and the product's host side (`lanelet2.lane_successors`, the lane table) against the model.  No GPU."""
import math
import os

import numpy as np
import pytest

import lane_follow_model as lf
from conftest import GOLDEN

F32 = np.float32


@pytest.fixture(scope='module')
def maps():
    from torchdrivesim_amd import lanelet2
    return {k: lanelet2.load_lanelet_map(os.path.join(GOLDEN, f), origin=(0.0, 0.0))
            for k, f in (('Town01', 'carla_Town01.osm.gz'), ('Town02', 'carla_Town02.osm.gz'), ('testing', 'testing_lanelet2map.osm'))}


@pytest.fixture(scope='module')
def town01(maps):
    return lf.Lanes(maps['Town01'])


def straight_map(length=400.0, pieces=1):
    """`pieces` lanelets of equal length in a row on the x axis, joined through shared bound point ids"""
    from torchdrivesim_amd import lanelet2
    xs = np.linspace(0.0, length, pieces + 1)
    out = []
    for i in range(pieces):
        left = np.array([[xs[i], 1.75, 0.0], [xs[i + 1], 1.75, 0.0]])
        right = np.array([[xs[i], -1.75, 0.0], [xs[i + 1], -1.75, 0.0]])
        out.append(lanelet2.Lanelet(i + 1, left, right, np.array([2 * i, 2 * i + 2]), np.array([2 * i + 1, 2 * i + 3]), {'type': 'lanelet'}))
    return lanelet2.LaneletMap([], np.zeros((0, 3)), out)


def scene_of(state, size, extra_boxes=(), extra_speed=()):
    """entities = the extra boxes first, then the NPCs: (boxes, sc, speed, present, self_index)"""
    extra = np.array(extra_boxes, F32).reshape(-1, 5)
    boxes = np.concatenate([extra, np.concatenate([state[:, :2], size, state[:, 2:3]], 1)], 0).astype(F32)
    sc = np.stack([np.sin(boxes[:, 4]), np.cos(boxes[:, 4])], 1).astype(F32)
    speed = np.concatenate([np.array(extra_speed, F32).reshape(-1), state[:, 3]]).astype(F32)
    return boxes, sc, speed, np.ones(len(boxes), bool), np.arange(len(extra), len(boxes))


# ---------------------------------------------------------------------------------------------------------------- lane graph
@pytest.mark.parametrize('name, lanelets, one, two', [('Town01', 124, 88, 36), ('Town02', 88, 64, 24)])
def test_successor_counts_of_the_shipped_maps(maps, name, lanelets, one, two):
    from torchdrivesim_amd import lanelet2
    for m in (maps[name], lanelet2.revert_map(maps[name])):
        start, items = lanelet2.lane_successors(m)
        assert start.dtype == np.int32 and items.dtype == np.int32 and start.shape == (lanelets + 1,) and start[-1] == len(items)
        counts = np.diff(start)
        assert ((counts == 1).sum(), (counts == 2).sum(), (counts == 0).sum()) == (one, two, 0)
        rows = [list(items[start[i]:start[i + 1]]) for i in range(lanelets)]
        assert rows == lf.successors(m)                                    # the product's hash join == the model's double loop
        assert all(i not in r and r == sorted(r) for i, r in enumerate(rows))
        table = lanelet2.lane_table(m)
        assert np.array_equal(table.succ_start, start) and np.array_equal(table.succ_items, items)


def test_dead_ends_of_the_small_map(maps):
    """the three lanelets of testing_lanelet2map.osm share no bound end points: each of them is a dead end"""
    from torchdrivesim_amd import lanelet2
    m = maps['testing']
    start, items = lanelet2.lane_successors(m)
    assert [l.id for l, n in zip(m.laneletLayer, np.diff(start)) if n == 0] == [-9, -14, -19] and len(items) == 0
    assert lf.successors(m) == [[], [], []]


def test_a_lanelet_with_an_empty_bound_is_outside_the_graph():
    from torchdrivesim_amd import lanelet2
    m = straight_map(30.0, 3)
    mid = m.laneletLayer[1]
    m.laneletLayer[1] = lanelet2.Lanelet(mid.id, mid.left[:0], mid.right, mid.left_ids[:0], mid.right_ids, {})
    start, items = lanelet2.lane_successors(m)
    assert list(np.diff(start)) == [0, 0, 0] and lf.successors(m) == [[], [], []]


# ---------------------------------------------------------------------------------------------------------------- snap
def test_snap_recovers_points_drawn_on_centre_lines(town01):
    """along the lane, a point of a centre line comes back with its lanelet and arc length -- also in junctions, where several lanelets contain
    it and the heading decides; arcs right at a lanelet's two ends (the joints) included"""
    g = np.random.default_rng(3)
    checked = junction = joints = 0
    for l in list(g.choice(len(town01), 40, replace=False)):
        length = town01.length(l)
        for s in (0.0, length, float(g.uniform(0.05, 0.95)) * length):
            x, y, psi, sn, cs = town01.pose(l, s)
            lane, arc, lateral, scores = lf.snap(town01, x, y, sn, cs, with_scores=True)
            ranked = sorted((sc for _, sc, _ in scores if sc is not None), reverse=True)
            assert abs(float(lateral)) < 1e-3
            if s in (0.0, length):
                # a joint: the point is the end of one lanelet and the start of the next (or of both branches of a fork), all of them along the
                # heading; the lowest index among them wins, and the arc is that lanelet's own end
                assert lane >= 0 and ranked[0] > 1 - 1e-6 and min(abs(arc), abs(arc - town01.length(lane))) < 1e-3
                assert lane == l or l in town01.succ[lane] or lane in town01.succ[l] or set(town01.succ[lane]) & set(town01.succ[l]) or \
                    any(lane in town01.succ[p] and l in town01.succ[p] for p in range(len(town01)))
                joints += 1
                continue
            if len(ranked) > 1 and ranked[0] - ranked[1] < 1e-6:
                assert lane <= l                       # lanelets that fork from one stem share their first stretch: the lowest index wins
                continue
            assert lane == l and abs(arc - s) < 1e-3, (l, s, lane, arc, lateral)
            checked += 1
            junction += len(ranked) > 1
    print('recovered', checked, 'of them where lanelets overlap', junction, 'at joints, in the neighbour', joints)
    assert checked >= 35 and junction >= 10 and joints == 80


def test_snap_takes_the_lanelet_the_heading_agrees_with(town01):
    """in overlapping junction lanelets the same point belongs to the lanelet it is driving along"""
    found = 0
    for l in range(len(town01)):
        s = town01.length(l) / 2
        x, y, psi, sn, cs = town01.pose(l, s)
        _, _, _, scores = lf.snap(town01, x, y, sn, cs, with_scores=True)
        others = [(k, sc) for k, sc, _ in scores if sc is not None and k != l and 0.1 < sc < 0.95]
        if not others:
            continue
        k = others[0][0]                                                      # another lanelet over the same ground, at an angle
        kk, u, tx, ty = lf.foot(town01.cl[k], float(x), float(y))
        lane, _, _ = lf.snap(town01, x, y, F32(ty), F32(tx))                 # the same point, heading along THAT lanelet
        assert lane == k or lf.snap(town01, x, y, F32(ty), F32(tx), with_scores=True)[3][0][1] >= 1 - 1e-6
        assert lf.snap(town01, x, y, sn, cs)[0] == l
        found += 1
        if found == 5:
            break
    assert found == 5


def test_a_pose_against_every_candidate_is_not_snapped(town01):
    misses = 0
    for l in range(0, len(town01), 7):
        x, y, psi, sn, cs = town01.pose(l, town01.length(l) / 2)
        lane, arc, lateral, scores = lf.snap(town01, x, y, F32(-sn), F32(-cs), with_scores=True)
        if all(sc is None or sc > 0 for _, sc, _ in lf.snap(town01, x, y, sn, cs, with_scores=True)[3]):
            assert lane == -1 and arc == 0.0            # every lanelet here runs with the pose: turned round, it runs against all of them
            misses += 1
    assert misses >= 5
    assert lf.snap(town01, F32(1e6), F32(1e6), F32(0), F32(1))[0] == -1


# ---------------------------------------------------------------------------------------------------------------- IDM
def test_a_free_road_step_is_the_closed_form():
    lanes = lf.Lanes(straight_map())
    v, v0, dt = 5.0, 8.0, 0.1
    r = lf.step_npc(lanes, 0, 10.0, 0, F32(v), (F32(4.97), F32(2.04)), F32(v0), np.zeros((0, 5), F32), np.zeros((0, 2), F32), np.zeros(0, F32),
                    np.zeros(0, bool), -1, seed=1, scene_id=0, npc=0, dt=dt)
    dt = float(F32(dt))
    acc = 1.5 * (1.0 - (v / v0) ** 4)
    v_new = F32(v + acc * dt)
    assert r['leader'] == -1 and r['speed'] == v_new
    assert r['arc'] == 10.0 + (v + float(v_new)) / 2.0 * dt and r['lane'] == 0 and r['hops'] == 0
    assert (r['x'], r['y'], r['sin'], r['cos']) == (F32(r['arc']), F32(0), F32(0), F32(1))
    # at the desired speed nothing accelerates; above it the IDM brakes, but never harder than b_max
    assert lf.idm_acceleration(8.0, 8.0, -1, 0.0, 0.0) == 0.0
    assert lf.idm_acceleration(8.0, 8.0, 3, 0.05, 0.0) == -6.0
    # the fourth power is two squarings
    assert lf.idm_acceleration(3.0, 7.0, -1, 0.0, 0.0) == 1.5 * (1.0 - ((3.0 / 7.0) * (3.0 / 7.0)) * ((3.0 / 7.0) * (3.0 / 7.0)))


def test_a_queue_comes_to_rest_behind_a_standing_box():
    """five NPCs, 12 m apart at 8 m/s, a box standing 50 m ahead of the first; 400 steps of 0.1 s.  No two rectangles ever overlap, and the
    final gaps lie in [s0 - 0.05, s0 + 0.5]: the IDM's equilibrium gap at rest is s0 (measured on this model: 1.9999 m each)"""
    lanes = lf.Lanes(straight_map())
    N, s0, length = 5, 2.0, 4.97
    size = np.tile(np.array([length, 2.04], F32), (N, 1))
    lane, hops, arc = np.zeros(N, int), np.zeros(N, int), np.array([100.0 - 12.0 * i for i in range(N)])
    state = np.zeros((N, 4), F32)
    state[:, 0], state[:, 3] = arc, 8.0
    box = [150.0, 0.0, length, 2.04, 0.0]
    for _ in range(400):
        boxes, sc, speed, present, self_index = scene_of(state, size, [box], [0.0])
        out = lf.step_scene(lanes, lane, arc, hops, state, size, np.full(N, 8, F32), np.ones(N, bool), boxes, sc, speed, present, self_index, 1, 0, 0.1)
        lane, arc, hops, state = out['lane'], out['arc'], out['hops'], out['state']
        gaps = np.concatenate([[150.0], arc[:-1]]) - arc - length
        assert (gaps > 0).all()
    print('final gaps', gaps)
    assert (state[:, 3] == 0).all() and list(out['leader']) == [0, 1, 2, 3, 4]
    assert ((gaps >= s0 - 0.05) & (gaps <= s0 + 0.5)).all(), gaps


def free_step(lanes, lane, arc, hops, v, dt, seed=5, scene_id=2, npc=1):
    return lf.step_npc(lanes, lane, arc, hops, F32(v), (F32(4.97), F32(2.04)), F32(8), np.zeros((0, 5), F32), np.zeros((0, 2), F32),
                       np.zeros(0, F32), np.zeros(0, bool), -1, seed=seed, scene_id=scene_id, npc=npc, dt=dt)


def test_a_hop_keeps_the_travelled_distance():
    lanes = lf.Lanes(straight_map(400.0, 40))                               # lanelets of 10 m
    r = free_step(lanes, 3, 9.7, 0, 8.0, 0.1)
    assert (r['lane'], r['hops']) == (4, 1)
    before, after = 3 * 10.0 + 9.7, r['lane'] * 10.0 + r['arc']
    assert abs(after - (before + r['ds'])) < 1e-12


def test_several_hops_in_one_step():
    lanes = lf.Lanes(straight_map(400.0, 80))                               # lanelets of 5 m; 8 m/s for 2 s = 16 m
    r = free_step(lanes, 10, 1.0, 2, 8.0, 2.0)
    assert (r['lane'], r['hops']) == (13, 5) and abs(r['lane'] * 5.0 + r['arc'] - (51.0 + r['ds'])) < 1e-12


def test_a_dead_end_stops_the_npc_at_the_lanelets_end():
    lanes = lf.Lanes(straight_map(40.0, 2))
    r = free_step(lanes, 1, 19.9, 1, 8.0, 0.1)
    assert (r['lane'], r['arc'], r['speed'], r['hops']) == (1, 20.0, F32(0), 1) and r['x'] == F32(40)
    # seen from further back, the end of the lane is what the NPC brakes for
    far = free_step(lanes, 1, 5.0, 1, 8.0, 0.1)
    assert far['leader'] == -2 and far['speed'] < F32(8)
    pieces, smin, total, dead, chain = lf.build_path(lanes, 0, 15.0, 0, 5, 2, 1, 60.0)
    assert dead and chain == [0, 1] and total == 25.0 and pieces[0][0] + smin == 15.0       # (the centre line has a point every 10 m)


def test_the_path_ends_where_the_horizon_is_covered(town01):
    pieces, smin, total, dead, chain = lf.build_path(town01, 0, 1.0, 0, 9, 4, 2, 60.0)
    assert not dead and 60.0 <= total and pieces[-1][5] < 60.0 and len(chain) <= lf.MAX_HOPS + 1 and len(pieces) <= lf.MAX_PIECES
    assert all(b in town01.succ[a] for a, b in zip(chain[:-1], chain[1:]))


def test_the_vectorised_projection_is_the_scalar_one(town01):
    g = np.random.default_rng(11)
    pieces, smin, total, dead, _ = lf.build_path(town01, 5, 3.0, 0, 1, 0, 0, 60.0)
    x0, y0 = pieces[0][0], pieces[0][1]
    px, py = x0 + g.uniform(-40, 40, 200), y0 + g.uniform(-40, 40, 200)
    d, d2, bi = lf.project_all(pieces, smin, px, py)
    for k in range(200):
        assert lf.project(pieces, smin, float(px[k]), float(py[k])) == (d[k], d2[k], bi[k])


# ---------------------------------------------------------------------------------------------------------------- route stream
def test_philox_known_answers():
    """the Random123 answers tests/test_spawn_model.py holds spawn's generator to"""
    h = lambda s: tuple(int(w, 16) for w in s.split())
    assert lf.philox4x32_10((0, 0, 0, 0), (0, 0)) == h('6627e8d5 e169c58d bc57ac4c 9b00dbd8')
    ones = 0xFFFFFFFF
    assert lf.philox4x32_10((ones,) * 4, (ones, ones)) == h('408f276d 41c83b0e a20bc7c6 6d5451fd')
    assert lf.philox4x32_10(h('243f6a88 85a308d3 13198a2e 03707344'), h('a4093822 299f31d0')) == h('d16cfe09 94fdcceb 5001e420 24126ea1')


def test_the_route_stream_is_its_own_and_counts_scene_npc_hop(town01):
    import spawn_model as sm
    seed, scene = 0x0123456789ABCDEF, (5 << 32) | 7
    assert lf.route_word(seed, scene, 3, 11) == lf.philox4x32_10((7, 5, 3, 11), (0x89ABCDEF ^ 0x4C414E45, 0x01234567 ^ 0x464F4C57))[0]
    assert lf.route_word(seed, scene, 3, 11) != sm.draw(seed, scene, 3, 11)[0]
    fork = next(l for l in range(len(town01)) if len(town01.succ[l]) == 2)
    grid = [(s, b, n, h) for s in (1, 2) for b in (0, 9) for n in (0, 1, 2) for h in range(6)]
    picks = {k: town01.successor(fork, *k) for k in grid}
    assert set(picks.values()) == set(town01.succ[fork])                    # both branches are taken
    # each of the four arguments matters: somewhere on the grid, changing it alone changes the branch
    for pos in range(4):
        assert any(picks[k] != picks[q] for k in grid for q in grid if k[pos] != q[pos] and k[:pos] + k[pos + 1:] == q[:pos] + q[pos + 1:]), pos
    # and nothing else does: the pick equals the draw stated in the header, whatever lanelet asks and wherever the NPC stands
    for k in grid:
        want = town01.succ[fork][(lf.philox4x32_10((k[1], 0, k[2], k[3]), (k[0] ^ 0x4C414E45, 0x464F4C57))[0] * 2) >> 32]
        assert picks[k] == want
    # a path is the same wherever it is built from: hop h of an NPC is one draw
    _, _, _, _, chain = lf.build_path(town01, fork, 0.0, 4, 1, 9, 2, 500.0)
    assert chain[1] == picks[(1, 9, 2, 4)]
