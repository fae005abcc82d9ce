"""The float64 model of routes to a destination (tests/route_to_model.py) against what it has to get right on its own: a distance
table that equals an independent Dijkstra bit for bit, routes that follow the lane graph and are as long as the shortest path, the cases of the
definition (same lanelet ahead and behind, b = 0, b = len, a tie, dead ends, truncation at 16 lanelets and its continuation).  Maps: the ring
with a fork, a diamond whose fork is an exact tie, the three unconnected lanelets of testing_lanelet2map.osm, Town01 and Town02.  No GPU.

Figures of the towns with the tables' real lengths (printed by test_the_figures_of_the_towns, asserted there):
  Town01: 124 lanelets, 160 edges, at most 2 successors, strongly connected; shortest paths over all ordered pairs: median 12 lanelets,
          at most 27, both ends counted; 13 216 of 15 252 pairs (86.7 %) fit in 16 lanelets, 2 036 (13.3 %) do not.
  Town02:  88 lanelets, 112 edges, at most 2 successors, strongly connected; median 11, at most 25; 7 054 of 7 656 pairs (92.1 %) fit.
  Town01, every ordered pair from arc 0 to arc 0: 1 319 of 15 252 routes (8.6 %) are truncated (a destination at arc 0 needs one lanelet fewer).
  length + rest against the table's shortest distance, 3 000 random pairs a town: at most 4 ulp apart (the bound is the number of pieces)."""
import math
import os

import numpy as np
import pytest

import route_model as rm
import route_to_model as rt
from conftest import GOLDEN

INF = math.inf


@pytest.fixture(scope='module')
def lanes():
    """name -> (model, its distance table)"""
    from torchdrivesim_amd import lanelet2
    out = {k: rm.Lanes(lanelet2.load_lanelet_map(os.path.join(GOLDEN, f), origin=(0.0, 0.0)))
           for k, f in (('Town01', 'carla_Town01.osm.gz'), ('Town02', 'carla_Town02.osm.gz'), ('testing', 'testing_lanelet2map.osm'))}
    out['ring'] = rm.Lanes(rm.ring_with_fork())
    out['diamond'] = rm.Lanes(rt.diamond())
    return {k: (m, rt.distance_table(m)) for k, m in out.items()}


def ulp(x):
    return float(np.spacing(np.float64(abs(x))))


def path_lanelets(model, table, l0, t):
    """lanelets on the shortest path from the start of l0 to the START of t, l0 included, t not"""
    count, l = 0, l0
    while True:
        count += 1
        l = min((s for s in model.succ[l] if rt.usable(model, s)), key=lambda s: table[t][s])
        if l == t:
            return count
        assert count <= len(model)


def check_route(model, table, l0, a0, t, b, route, rest):
    """what every dealt route has to satisfy; `length + rest` against the shortest distance the table gives.  Both are sums of the same numbers
    -- (len(l0) - a0), the lengths of the lanelets in between, b and, for a truncated route, ONE table entry -- in a different association:
    front to back here, back to front in the table.  A complete route of n pieces makes n - 1 additions on either side, each wrong by at most
    half an ulp of a partial sum <= total: within n ulp(total).  (A truncated one makes 17; the bound stays n = 16.)"""
    assert route.lanes[0] == l0 and route.start_arc == a0
    for x, y in zip(route.lanes, route.lanes[1:]):
        assert y in model.succ[x] and rt.usable(model, y), 'consecutive route lanelets are graph edges'
    total = 0.0
    for j in range(route.n):
        assert route.offsets[j] == total
        lo, hi = route.interval(model, j)
        assert 0.0 <= lo <= hi <= model.length(route.lanes[j])
        total = total + (hi - lo)
    assert route.length == total and route.n <= rt.MAX_LANES
    if t == l0 and b >= a0:
        want = b - a0
    else:
        want = (model.length(l0) - a0) + min(table[t][s] for s in model.succ[l0] if rt.usable(model, s)) + b
    err = abs((route.length + rest) - want)
    assert err <= route.n * ulp(want), (l0, a0, t, b, route.length, rest, want)
    if rest == 0.0:
        assert route.lanes[-1] == t and route.end_arc == b or (b == 0.0 and t in model.succ[route.lanes[-1]])
    else:
        assert route.n == rt.MAX_LANES and route.end_arc == model.length(route.lanes[-1]) and 0.0 < rest < INF
    return err / ulp(want)


def test_the_fixtures_are_what_the_tests_take_them_for(lanes):
    ring, _ = lanes['ring']
    assert ring.succ == [[1, 4], [2], [3], [0], []]
    d, table = lanes['diamond']
    assert d.succ == [[1, 2], [3], [3], [0]]
    assert np.float64(d.length(1)).tobytes() == np.float64(d.length(2)).tobytes(), 'the legs are bit-equal: the fork is an exact tie'
    assert d.cum[1] == d.cum[2] and d.length(1) == math.sqrt(34.0) + math.sqrt(34.0)
    assert table[3][1] == table[3][2] == d.length(1) and table[0][1] == table[0][2]
    testing, _ = lanes['testing']
    assert len(testing) == 3 and testing.succ == [[], [], []]
    assert rt.MAX_GRAPH == 2048 and rt.MAX_LANES == 16


@pytest.mark.parametrize('name', ['ring', 'diamond', 'testing', 'Town01', 'Town02'])
def test_the_table_equals_dijkstra_bit_for_bit(lanes, name):
    model, table = lanes[name]
    assert table.tobytes() == rt.dijkstra(model).tobytes()
    L = len(model)
    for t in range(L):
        assert table[t][t] == (0.0 if rt.usable(model, t) else INF)
    for l in range(L):
        if not rt.usable(model, l):
            assert np.isinf(table[l]).all() and np.isinf(table[:, l]).all()
    if name == 'ring':
        assert np.isinf(table[:4, 4]).all() and table[4][4] == 0.0, 'nothing but itself is reachable from the dead end'
        assert table[4].tolist() == [20.0, 80.0, 60.0, 40.0, 0.0], 'but it is reachable'
        assert table[0].tolist() == [0.0, 60.0, 40.0, 20.0, INF]
    if name == 'testing':
        assert np.isinf(table).sum() == 6 and (np.diag(table) == 0.0).all()


def test_the_figures_of_the_towns(lanes):
    """graph sizes and shortest paths over all ordered pairs, with the tables' real lengths (the module docstring records them)"""
    want = {'Town01': (124, 160, 12, 27, 13216, 15252), 'Town02': (88, 112, 11, 25, 7054, 7656)}
    for name, figures in want.items():
        model, table = lanes[name]
        L = len(model)
        assert all(rt.usable(model, l) for l in range(L)) and np.isfinite(table).all(), 'strongly connected'
        assert max(len(s) for s in model.succ) == 2
        # lanelets on the way from the start of l0 to the start of t, both counted: a route from arc 0 to arc 0+ holds that many
        counts = [path_lanelets(model, table, l0, t) + 1 for l0 in range(L) for t in range(L) if l0 != t]
        got = (L, sum(len(s) for s in model.succ), int(np.median(counts)), max(counts), sum(c <= rt.MAX_LANES for c in counts), len(counts))
        print(name, got, f'{100.0 * got[4] / got[5]:.1f} % fit')
        assert got == figures, got


@pytest.mark.parametrize('name', ['ring', 'diamond', 'Town01', 'Town02'])
def test_random_routes_are_shortest_paths(lanes, name):
    model, table = lanes[name]
    g = np.random.default_rng(5)
    ok = [l for l in range(len(model)) if rt.usable(model, l)]
    worst = complete = cut = 0
    for _ in range(3000 if name.startswith('Town') else 300):
        l0, t = int(g.choice(ok)), int(g.choice(ok))
        a0, b = float(g.uniform(0, 1)) * model.length(l0), float(g.uniform(0, 1)) * model.length(t)
        route, rest = rt.deal(model, table, l0, a0, t, b)
        if name == 'ring' and l0 == 4:
            assert (route.n, rest) == ((1, 0.0) if t == 4 and b >= a0 else (0, INF))
            continue
        assert route.n >= 1, (l0, a0, t, b)
        worst = max(worst, check_route(model, table, l0, a0, t, b, route, rest))
        complete, cut = complete + (rest == 0.0), cut + (rest > 0.0)
    print(name, 'worst |length + rest - shortest| =', worst, 'ulp;', complete, 'complete,', cut, 'truncated')
    assert complete > 0 and (cut > 100 if name.startswith('Town') else cut == 0)


def test_the_cases_of_the_definition_on_the_ring(lanes):
    ring, table = lanes['ring']
    deal = lambda *a, **k: rt.deal(ring, table, *a, **k)
    r, rest = deal(1, 5.0, 1, 12.5)                                          # ahead on the same lanelet: one piece
    assert (r.lanes, r.start_arc, r.end_arc, r.offsets, r.length, rest) == ([1], 5.0, 12.5, [0.0], 7.5, 0.0)
    r, rest = deal(1, 12.5, 1, 5.0)                                          # behind: round the ring
    assert (r.lanes, r.start_arc, r.end_arc, r.length, rest) == ([1, 2, 3, 0, 1], 12.5, 5.0, 72.5, 0.0)
    assert r.offsets == [0.0, 7.5, 27.5, 47.5, 67.5]
    r, rest = deal(1, 5.0, 1, 5.0)                                           # at the destination: a route of zero length is no route
    assert (r.n, rest) == (0, 0.0)
    r, rest = deal(1, 5.0, 2, 0.0)                                           # b = 0: nothing is appended, the route ends at the lanelet's end
    assert (r.lanes, r.end_arc, r.length, rest) == ([1], 20.0, 15.0, 0.0)
    r, rest = deal(1, 5.0, 3, 0.0)
    assert (r.lanes, r.end_arc, r.length, rest) == ([1, 2], 20.0, 35.0, 0.0)
    r, rest = deal(1, 5.0, 2, 20.0)                                          # b = len
    assert (r.lanes, r.end_arc, r.length, rest) == ([1, 2], 20.0, 35.0, 0.0)
    r, rest = deal(1, 5.0, 2, 99.0)                                          # clamped to len; arcs below 0 and NaN to 0
    assert (r.lanes, r.end_arc, r.length) == ([1, 2], 20.0, 35.0)
    assert deal(1, -3.0, 2, math.nan)[0].length == 20.0 and deal(1, 99.0, 2, 1.0)[0].length == 1.0
    r, rest = deal(3, 2.0, 4, 7.0)                                           # into the dead end
    assert (r.lanes, r.length, rest) == ([3, 0, 4], 45.0, 0.0)
    for t in range(4):                                                       # out of it: nowhere
        for b in (0.0, 1.0):
            assert (deal(4, 3.0, t, b)[0].n, deal(4, 3.0, t, b)[1]) == (0, INF)
    assert deal(4, 3.0, 4, 9.0)[0].lanes == [4] and deal(4, 9.0, 4, 3.0)[0].n == 0 and deal(4, 9.0, 4, 3.0)[1] == INF
    for bad in ((-1, 0.0, 1, 0.0), (5, 0.0, 1, 0.0), (1, 0.0, -1, 0.0), (1, 0.0, 7, 0.0)):      # lanes out of range
        assert deal(*bad)[0].n == 0 and deal(*bad)[1] == INF
    assert deal(1, 5.0, 2, 1.0, present=False)[1] == INF and rt.deal(None, None, 1, 5.0, 2, 1.0)[1] == INF


def test_the_tie_at_the_diamond_takes_the_first_successor(lanes):
    d, table = lanes['diamond']
    r, rest = rt.deal(d, table, 0, 2.0, 3, 4.0)
    assert (r.lanes, rest) == ([0, 1, 3], 0.0) and r.length == (8.0 + d.length(1)) + 4.0
    r, rest = rt.deal(d, table, 3, 1.0, 0, 0.0)                              # b = 0 straight after the start
    assert (r.lanes, r.end_arc, rest) == ([3], d.length(3), 0.0)
    r, rest = rt.deal(d, table, 2, 1.0, 1, 1.0)                              # from one leg to the other: round
    assert (r.lanes, rest) == ([2, 3, 0, 1], 0.0)


def test_unconnected_lanelets_reach_only_themselves(lanes):
    model, table = lanes['testing']
    for l0 in range(3):
        for t in range(3):
            r, rest = rt.deal(model, table, l0, 1.0, t, 2.0)
            assert (r.n, rest) == ((1, 0.0) if l0 == t else (0, INF))
        behind = rt.deal(model, table, l0, 2.0, l0, 1.0)
        assert (behind[0].n, behind[1]) == (0, INF), 'behind on a lanelet without successors'


def test_truncated_routes_of_town01_continue_to_their_destination(lanes):
    """All ordered pairs of Town01 from arc 0 to arc 0: 1 319 of 15 252 routes (8.6 %) are truncated -- a destination at arc 0 ends the route on
    the lanelet before it, so these are the pairs more than 17 lanelets apart with both ends counted; for destinations inside their lanelet it is
    the 13.3 % of the module docstring.  Every truncated route is continued from its end by a second deal, which reaches the destination, and the two lengths
    add up to the first deal's length + rest."""
    model, table = lanes['Town01']
    L = len(model)
    cut = pairs = 0
    for l0 in range(L):
        for t in range(L):
            if l0 == t:
                continue
            pairs += 1
            first, rest = rt.deal(model, table, l0, 0.0, t, 0.0)
            assert first.n >= 1
            if rest == 0.0:
                continue
            cut += 1
            assert first.n == 16 and first.end_arc == model.length(first.lanes[-1])
            second, rest2 = rt.deal(model, table, first.lanes[-1], first.end_arc, t, 0.0)
            assert rest2 == 0.0 and second.n <= 12 and second.lanes[0] == first.lanes[-1] and second.offsets[1] == 0.0, 'piece 0 has no length'
            assert t in model.succ[second.lanes[-1]]
            whole = first.length + rest
            assert abs((first.length + second.length) - whole) <= (first.n + second.n) * ulp(whole)
    print(f'Town01: {cut} of {pairs} routes from arc 0 to arc 0 are truncated ({100.0 * cut / pairs:.1f} %)')
    assert (cut, pairs) == (1319, 15252)
