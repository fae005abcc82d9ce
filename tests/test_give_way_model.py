"""What the model of giving way at junctions (tests/give_way_model.py) must get right on its own, before any kernel is held to it: the
conflicts of the shipped maps, a synthetic crossing one can count by hand, and the behaviour -- four NPCs that arrive at a crossing together collide
without the option and take turns with it.  CPU only."""
import os

import numpy as np
import pytest

import give_way_cases as gc
import give_way_model as gw
import lane_follow_model as lf
from conftest import GOLDEN

F32 = np.float32


@pytest.fixture(scope='module')
def crossing():
    model = lf.Lanes(gc.crossing_map())
    return model, gw.conflict_tables(model)


# ---------------------------------------------------------------------------------------------------------------- the shipped maps
@pytest.mark.parametrize('name, file, lanelets, conflicted, pairs, most', [('Town01', 'carla_Town01.osm.gz', 124, 72, 144, 3), ('Town02', 'carla_Town02.osm.gz', 88, 48, 96, 3),
                                                                           ('testing', 'testing_lanelet2map.osm', 3, 0, 0, 0)])
def test_conflicts_of_the_shipped_maps(name, file, lanelets, conflicted, pairs, most):
    from torchdrivesim_amd import lanelet2
    stored = lanelet2.load_lanelet_map(os.path.join(GOLDEN, file), origin=(0.0, 0.0))
    for m in (stored, lanelet2.revert_map(stored)):
        model = lf.Lanes(m)
        exit_, zone_in, zone_out = gw.conflict_tables(model)
        C = gw.conflicting((exit_, zone_in, zone_out))
        assert (len(model), int(C.any(1).sum()), int(C.sum()), int(C.sum(1).max(initial=0))) == (lanelets, conflicted, pairs, most)
        assert np.array_equal(exit_ >= 0, (exit_ >= 0).T), 'the relation is symmetric before it is made so'
        same_stream = gw.excluded(model)
        for a, b in np.argwhere(exit_ >= 0).tolist():
            assert b not in same_stream[a] and a not in same_stream[b]
            assert a != b and b not in model.succ[a] and a not in model.succ[b] and not any(a in s and b in s for s in model.succ)
        for a in np.nonzero(C.any(1))[0]:
            assert len(model.succ[a]) == 1 and 11.0 < model.length(a) < 24.5, 'a junction lanelet'
            assert 0.0 <= zone_in[a] <= zone_out[a] <= model.length(a) and zone_out[a] == exit_[a].max()
        quiet = ~(exit_ >= 0).any(1)
        assert np.isinf(zone_in[quiet]).all() and (zone_out[quiet] == -1).all()


def test_the_pair_counts_at_other_clearances():
    """a narrower clearance or a finer step finds the same pairs; at 2.5 m Town02 gains one pair (lanelets 41 and 61, two turns of one junction
    that pass 2.0 - 2.5 m from each other), Town01 none"""
    from torchdrivesim_amd import lanelet2
    model = lf.Lanes(lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'carla_Town02.osm.gz'), origin=(0.0, 0.0)))
    for clearance, step, pairs in ((1.5, 0.5, 96), (1.5, 0.25, 96), (2.5, 0.5, 98)):
        assert int(gw.conflicting(gw.conflict_tables(model, clearance, step)).sum()) == pairs


# ---------------------------------------------------------------------------------------------------------------- the synthetic crossing
def test_the_crossing_by_hand(crossing):
    """lanelets 3 d + (0, 1, 2) = approach, junction, exit of stream d (east, north, west, south): see give_way_cases.crossing_map"""
    model, (exit_, zone_in, zone_out) = crossing
    assert model.succ == [[1], [2], [], [4], [5], [], [7], [8], [], [10], [11], []]
    C = gw.conflicting((exit_, zone_in, zone_out))
    assert np.argwhere(C).tolist() == [[1, 4], [1, 10], [4, 1], [4, 7], [7, 4], [7, 10], [10, 1], [10, 7]], 'crossing streams conflict, opposite ones do not'
    for d in range(4):
        j, from_right, from_left = 3 * d + 1, 3 * ((d + 1) % 4) + 1, 3 * ((d + 3) % 4) + 1
        assert (zone_in[j], zone_out[j]) == (3.5, 10.5)
        assert exit_[j, from_left] == 7.0 and exit_[j, from_right] == 10.5
    assert (exit_ >= 0).sum() == 8


def place(model, rows):
    """rows of (lanelet, arc, speed) -> the arrays give_way takes"""
    lane, arc = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float64)
    return lane, arc, np.zeros(len(rows), np.int32), np.array([r[2] for r in rows], F32), np.tile(np.array(gc.SIZE, F32), (len(rows), 1)), np.ones(len(rows), bool)


def test_an_exact_tie_goes_to_the_lower_index(crossing):
    """two approaches that are each other turned by a quarter turn: D, length and speed are bit-equal, so are the times"""
    model, tables = crossing
    for rows, want in (([(0, 40.0, 6.0), (3, 40.0, 6.0)], [-1, 0]), ([(3, 40.0, 6.0), (0, 40.0, 6.0)], [-1, 0]), ([(9, 40.0, 6.0), (6, 40.0, 6.0), (0, 40.0, 6.0)], [-1, 0, 0])):
        stop_at, yield_to, s = gw.give_way(model, tables, *place(model, rows), 1, 0)
        assert all(x['t'] == s[0]['t'] and x['D'] == 23.5 and not x['committed'] for x in s)
        assert yield_to.tolist() == want and [np.isfinite(x) for x in stop_at] == [y >= 0 for y in want] and set(stop_at[yield_to >= 0]) == {23.5}
    # a hair sooner beats the index
    _, yield_to, _ = gw.give_way(model, tables, *place(model, [(0, 40.0, 6.0), (3, 40.0 + 2.0 ** -40, 6.0)]), 1, 0)
    assert yield_to.tolist() == [1, -1]
    # opposite streams do not contend
    assert gw.give_way(model, tables, *place(model, [(0, 40.0, 6.0), (6, 41.0, 6.0)]), 1, 0)[1].tolist() == [-1, -1]


def test_an_npc_that_cannot_stop_is_committed(crossing):
    """D = 63.5 - arc, gap = D - 2.25; at 12 m/s and b_max = 6 the NPC stops within 12 m"""
    model, tables = crossing
    for arc, committed in ((49.0, False), (49.25, True), (55.0, True), (62.0, True)):          # gap 12.25, 12.0 (the bound itself), 6.25, -0.75
        s = gw.summary(model, tables, 0, arc, 0, 12.0, 4.5, 1, 0, 0, [], 60.0, 6.0, 1.0)
        assert s['junction'] == 1 and s['gap'] == 63.5 - arc - 2.25 and s['committed'] == committed
    # a committed NPC yields to nobody, and everybody yields to it, whatever the times and indices say
    stop_at, yield_to, s = gw.give_way(model, tables, *place(model, [(3, 58.0, 6.0), (0, 50.0, 12.0)]), 1, 0)
    assert s[1]['committed'] and not s[0]['committed'] and s[0]['t'] < s[1]['t'] and yield_to.tolist() == [1, -1]
    # two committed NPCs: nobody yields (the follow kernel's leader test is what is left)
    assert gw.give_way(model, tables, *place(model, [(3, 55.0, 12.0), (0, 55.0, 12.0)]), 1, 0)[1].tolist() == [-1, -1]
    # standing still: t is reckoned at the creep speed
    s = gw.summary(model, tables, 0, 40.0, 0, 0.0, 4.5, 1, 0, 0, [], 60.0, 6.0, 1.0)
    assert s['t'] == 21.25 and not s['committed']
    # beyond the horizon there is no junction yet; behind it none any more (zone_out = 10.5 on the junction lanelet, half a length is 2.25)
    assert gw.summary(model, tables, 0, 3.0, 0, 6.0, 4.5, 1, 0, 0, [], 60.0, 6.0, 1.0) is None
    assert gw.summary(model, tables, 0, 3.5, 0, 6.0, 4.5, 1, 0, 0, [], 60.0, 6.0, 1.0)['D'] == 60.0
    assert gw.summary(model, tables, 1, 12.5, 1, 6.0, 4.5, 1, 0, 0, [], 60.0, 6.0, 1.0)['committed']
    assert gw.summary(model, tables, 1, 12.75, 1, 6.0, 4.5, 1, 0, 0, [], 60.0, 6.0, 1.0) is None


def test_a_red_held_npc_does_not_stop_a_green_one(crossing):
    """NPC 0 (east) has the lower index at equal t, but stands before a red line 5 m ahead of it: NPC 1 (north) goes"""
    model, tables = crossing
    rows = place(model, [(0, 40.0, 6.0), (3, 40.0, 6.0)])
    red, green, elsewhere, behind, beyond = [(0, 47.0, True)], [(0, 47.0, False)], [(6, 47.0, True)], [(0, 39.0, True)], [(2, 5.0, True)]
    for lines, held, want in ((red, True, [-1, -1]), (green, False, [-1, 0]), (elsewhere, False, [-1, 0]), (behind, False, [-1, 0]), (beyond, False, [-1, 0]),
                              ([(1, 5.0, True)], True, [-1, -1])):                              # a line inside the junction, before the zone's end
        _, yield_to, s = gw.give_way(model, tables, *rows, 1, 0, lines=lines)
        assert s[0]['held'] == held and not s[1]['held'] and yield_to.tolist() == want, lines
    # NPC 0 itself still gives way to others while it is held
    _, yield_to, s = gw.give_way(model, tables, *place(model, [(3, 40.0, 6.0), (0, 40.0, 6.0)]), 1, 0, lines=red)
    assert s[1]['held'] and yield_to.tolist() == [-1, 0]
    # a committed NPC is never held
    _, _, s = gw.give_way(model, tables, *place(model, [(0, 55.0, 12.0)]), 1, 0, lines=[(0, 59.0, True)])
    assert s[0]['committed'] and not s[0]['held']


def test_an_npc_is_released_once_the_other_has_cleared_the_zone(crossing):
    """NPC 1 (north, junction lanelet 4) waits for NPC 0 (east, on junction lanelet 1): exit[1][4] = 10.5, so NPC 0's rear clears the pair's zone when its
    centre is 2.25 m past arc 10.5"""
    model, tables = crossing
    for arc, waits in ((5.0, True), (12.5, True), (12.75, False), (13.5, False)):
        _, yield_to, s = gw.give_way(model, tables, *place(model, [(1, arc, 6.0), (3, 40.0, 6.0)]), 1, 0)
        assert yield_to.tolist() == [-1, 0 if waits else -1], arc
    # on the exit lanelet it has no junction at all
    assert gw.give_way(model, tables, *place(model, [(2, 1.0, 6.0), (3, 40.0, 6.0)]), 1, 0)[1].tolist() == [-1, -1]
    # against the stream from its left the zone ends sooner: exit[1][10] = 7.0
    for arc, waits in ((9.0, True), (9.25, False)):
        assert gw.give_way(model, tables, *place(model, [(1, arc, 6.0), (9, 40.0, 6.0)]), 1, 0)[1].tolist() == [-1, 0 if waits else -1]


# ---------------------------------------------------------------------------------------------------------------- behaviour
def run(model, tables, give_way, steps=300):
    """Four NPCs, one per stream, 25 m before the junction at 8 m/s, 300 steps of 0.1 s.  Simultaneous arrival is already enough to make them collide
    without the option (run here on the model: NPCs 0-1, 0-3, 1-2 and 2-3 overlap from step 39 on and stand in each other's way for good), so the
    starts are not shifted against each other."""
    scene = gc.Scene(model, [(3 * d, 35.0, 8.0) for d in range(4)], give_way=give_way, tables=tables)
    overlaps, waited = [], set()
    for it in range(steps):
        scene.step()
        overlaps += [(it,) + pair for pair in scene.overlaps()]
        waited |= set(np.nonzero(scene.leader == -3)[0].tolist())
    return scene, overlaps, waited


def test_four_npcs_at_a_crossing_take_turns(crossing):
    model, tables = crossing
    scene, overlaps, waited = run(model, tables, True)
    assert not overlaps, overlaps[:4]
    assert scene.lane.tolist() == [2, 5, 8, 11], 'all four have left the junction'
    assert len(waited) >= 3 and 0 not in waited, 'NPC 0 waits for nobody, the others for their turn'


def test_without_the_option_they_collide(crossing):
    model, tables = crossing
    scene, overlaps, waited = run(model, tables, False)
    assert overlaps and overlaps[0][0] < 60 and not waited
    assert {(i, j) for _, i, j in overlaps} == {(0, 1), (0, 3), (1, 2), (2, 3)}


def test_the_step_without_a_stop_is_the_follow_model(crossing):
    """stop_at = +inf: tests/lane_follow_model.py's step, every number"""
    model, tables = crossing
    scene = gc.Scene(model, [(0, 10.0, 6.0), (0, 30.0, 2.0), (4, 3.0, 5.0)], tables=tables)
    args = (scene.lane, scene.arc, scene.hops, scene.state, scene.size, scene.v0, scene.present, scene.boxes(), scene.sc, scene.state[:, 3].copy(), scene.present,
            np.arange(3), 1, 0, 0.1)
    want = lf.step_scene(model, *args)
    got = gw.step_scene(model, None, *args)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.isinf(got['stop_at']).all() and (got['yield_to'] == -1).all()
    r = gw.step_npc(model, 0, 10.0, 0, F32(6.0), scene.size[0], F32(8.0), scene.boxes()[:0], scene.sc[:0], scene.state[:0, 3], scene.present[:0], 0, 1, 0, 0, 0.1, 12.25)
    assert r['leader'] == -3 and r['speed'] < F32(6.0)
