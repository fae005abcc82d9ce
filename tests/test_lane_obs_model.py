"""
tests/lane_obs_model.py, the float64 model the lane-observation kernel (K8) equals bit for bit on the GPU, held to checks that do not share
its formulas -- distances against densely sampled centre lines, the selection against np.lexsort, the polylines against arc lengths measured
on the chain -- and to the cases of the definition (include/tdship.h "K8") worked out by hand on small synthetic maps.  CPU only.
"""
import math

import numpy as np
import pytest

import lane_obs_cases as cases
import lane_obs_model as lom

F32 = np.float32
INF = float('inf')


@pytest.fixture(scope='module')
def tables():
    maps = {name: make() for name, make in cases.STRUCTURES.items()}
    return {name: (m, lom.Lanes(m)) for name, m in maps.items()}


def sc_of(psi):
    return F32(math.sin(psi)), F32(math.cos(psi))


def see(lanes, x, y, psi=0.0, present=True, k=4, p=8, spacing=4.0, md=30.0):
    return lom.observe(lanes, (F32(x), F32(y)) + sc_of(psi), present, k, p, spacing, md)


# ------------------------------------------------------------------------------------------------------------------------
# 1. the independent check
# ------------------------------------------------------------------------------------------------------------------------
def sampled_distance(c, x, y, rounds=1):
    """the distance from (x, y) to the 2-D poly-line c by SAMPLING alone: 201 points per segment, then `rounds` - 1 times 201 points between
    the neighbours of the closest one (no projection anywhere)"""
    best = INF
    for a, b in zip(c[:-1, :2], c[1:, :2]):
        lo, hi = 0.0, 1.0
        for _ in range(rounds):
            t = np.linspace(lo, hi, 201)
            d = np.hypot(a[0] + t * (b[0] - a[0]) - x, a[1] + t * (b[1] - a[1]) - y)
            i = int(d.argmin())
            lo, hi = t[max(i - 1, 0)], t[min(i + 1, 200)]
        best = min(best, float(d.min()))
    return best


@pytest.mark.parametrize('name', sorted(cases.STRUCTURES))
def test_distances_selection_and_spacing_against_independent_checks(tables, name):
    lanelet_map, lanes = tables[name]
    rng = np.random.default_rng(sorted(cases.STRUCTURES).index(name))
    k, p, spacing, md = 4, 8, 4.0, 30.0
    for x, y, psi in cases.poses(rng, lanelet_map, 12):
        d2, sb = lom.feet(lanes, float(x), float(y))
        features, points, n_valid, index = see(lanes, x, y, psi, k=k, p=p, spacing=spacing, md=md)
        # distances: never above any sample, and within 1e-9 m of the best of a far finer sampling (distance is convex along a segment)
        for l in range(len(lanes)):
            if sb[l] < 0:
                assert not lom.usable(lanes, l)
                continue
            d = math.sqrt(d2[l])
            assert d <= sampled_distance(lanes.cl[l], float(x), float(y)) + 1e-12
            assert abs(d - sampled_distance(lanes.cl[l], float(x), float(y), rounds=7)) <= 1e-9
        # selection: np.lexsort on (l, float32(d2)) over the candidates in range
        cand = np.array([l for l in range(len(lanes)) if sb[l] >= 0 and d2[l] <= md * md], np.int64)
        order = cand[np.lexsort((cand, d2[cand].astype(F32)))][:k] if len(cand) else cand
        assert index.tolist() == order.tolist() + [-1] * (k - len(order))
        for slot, l in enumerate(order):
            assert features[slot, 7] == F32(math.sqrt(d2[l])) and n_valid[slot] >= 1
            # the polyline: consecutive valid points lie `spacing` apart along the chain of unique successors, measured on cum
            chain, cur = [l], l
            while len(lanes.succ[cur]) == 1 and len(chain) <= lom.MAX_HOPS:
                cur = lanes.succ[cur][0]
                chain.append(cur)
            starts = np.concatenate([[0.0], np.cumsum([lanes.length(c) for c in chain])])
            arc = float(features[slot, 4])                                   # (float32: only used to find the chain position roughly)
            previous = None
            for j in range(int(n_valid[slot])):
                # the model's own walk, checked against the chain laid out independently
                exact_arc = lanes.cum[l][sb[l]] + lom.segment_foot(lanes.cl[l], int(sb[l]), float(x), float(y))[5] * \
                    (lanes.cum[l][sb[l] + 1] - lanes.cum[l][sb[l]])
                assert abs(exact_arc - arc) <= 1e-5
                at = lom.walk(lanes, l, exact_arc + j * spacing)
                assert at is not None
                cur, pos = at
                hop = chain.index(cur) if chain.count(cur) == 1 else None
                wx, wy, seg, t = lom.point_at(lanes, cur, pos)
                on_cum = lanes.cum[cur][seg] + t * (lanes.cum[cur][seg + 1] - lanes.cum[cur][seg])
                assert abs(on_cum - pos) <= 1e-9 and -1e-12 <= t <= 1.0 + 1e-12
                a, b = lanes.cl[cur][seg][:2], lanes.cl[cur][seg + 1][:2]
                assert math.hypot(a[0] + t * (b[0] - a[0]) - wx, a[1] + t * (b[1] - a[1]) - wy) <= 1e-9
                if hop is not None:
                    along = starts[hop] + on_cum
                    assert abs(along - (exact_arc + j * spacing)) <= 1e-9
                    if previous is not None:
                        assert abs((along - previous) - spacing) <= 1e-9
                    previous = along
                # and the reported point is that world point in the observer's frame
                s, c = (float(v) for v in sc_of(psi))
                ex, ey = wx - float(x), wy - float(y)
                assert np.allclose(points[slot, j], [ex * c + ey * s, ey * c - ex * s], rtol=0, atol=1e-4)
            assert not points[slot, int(n_valid[slot]):].any()


def test_the_scalar_and_the_vectorised_foot_agree(tables):
    _, lanes = tables['dead_end']
    for x, y in [(3.0, 1.0), (12.0, 3.0), (-5.0, -5.0), (1e9, 2.0), (INF, 0.0)]:
        d2, sb = lom.feet(lanes, x, y)
        for l in range(len(lanes)):
            best, k = INF, -1
            for i in range(len(lanes.cl[l]) - 1):
                d = lom.segment_foot(lanes.cl[l], i, x, y)[8]
                if d < best:
                    best, k = d, i
            assert k == sb[l] and (k < 0 or best == d2[l])


# ------------------------------------------------------------------------------------------------------------------------
# 2. the definition's cases by hand
# ------------------------------------------------------------------------------------------------------------------------
def empty(out, k=4, p=8):
    features, points, n_valid, index = out
    return features.shape == (k, 8) and points.shape == (k, p, 2) and not features.any() and not points.any() and not n_valid.any() and \
        (index == -1).all()


def test_the_straight_lanelets_are_what_the_hand_cases_assume(tables):
    _, lanes = tables['chain']
    assert lanes.cl[0][:, 0].tolist() == [0.0, 5.0, 10.0] and lanes.cum[0] == [0.0, 5.0, 10.0]      # (the midpoints of the paired bound points)
    assert [lanes.length(l) for l in range(3)] == [10.0, 10.0, 10.0] and lanes.succ == [[1], [2], []]
    assert all(c[1] == 0.0 for l in range(3) for c in lanes.cl[l])
    assert tables['fork'][1].succ == [[1, 2], [], []] and tables['loop'][1].succ == [[1], [0]] and tables['tagged'][1].succ == [[2], [], [], []]
    assert tables['tagged'][1].flag == [False, True, True, False]


def test_empty_rows(tables):
    _, lanes = tables['chain']
    assert empty(see(lanes, 5, 1, present=False))                           # an absent observer
    assert empty(see(None, 5, 1))                                           # a scene without a map
    assert empty(see(lanes, math.nan, 1)) and empty(see(lanes, 5, math.nan)) and empty(see(lanes, 5, 1, psi=math.nan))     # a NaN pose
    assert empty(see(lanes, 5, 50, md=10.0))                                # nothing in range
    assert empty(see(lanes, INF, 0, md=INF))                                # no d2 below +inf: no candidate


def test_the_range_is_closed_and_exact(tables):
    _, lanes = tables['chain']
    out = see(lanes, 5, 3, md=3.0)                                          # d2 == r2 == 9: in range
    assert out[3].tolist() == [0, -1, -1, -1] and out[0][0, 7] == 3.0
    assert empty(see(lanes, 5, np.nextafter(F32(3), F32(4)), md=3.0))       # one binary32 step of the pose beyond
    _, short = tables['edge']
    d2, sb = lom.feet(short, 10.0, 10.0)
    assert d2[0] == np.nextafter(100.0, INF) and sb[0] == len(short.cl[0]) - 2                 # one binary64 step beyond r2 = 100 ...
    assert empty(see(short, 10, 10, md=10.0))                               # ... is out of range, though float32(d2) == 100
    assert F32(d2[0]) == F32(100.0) and see(short, 5, 10, md=10.0)[3][0] == 0
    assert lom.select(np.array([9.0, np.nextafter(9.0, INF)]), np.array([0, 0]), 4, 3.0) == [0]


def test_more_slots_than_candidates(tables):
    _, lanes = tables['chain']
    features, points, n_valid, index = see(lanes, 2, 1, k=6, md=INF)
    assert index.tolist() == [0, 1, 2, -1, -1, -1] and n_valid[3:].tolist() == [0, 0, 0] and not features[3:].any() and not points[3:].any()
    assert features[:3, 7].tolist() == [1.0, F32(math.sqrt(65.0)), F32(math.sqrt(325.0))]
    _, tagged = tables['tagged']
    assert see(tagged, 5, 2.9, k=6, md=INF)[3].tolist() == [0, 3, -1, -1, -1, -1]        # the tagged lanelets 1 and 2 are no candidates


def test_the_exact_tie_goes_to_the_lower_index(tables):
    _, lanes = tables['chain']
    d2, _ = lom.feet(lanes, 10.0, 3.0)
    assert d2[0] == d2[1] == 9.0                                            # the shared end point of 0 and its successor
    features, _, _, index = see(lanes, 10, 3)
    assert index.tolist() == [0, 1, 2, -1] and features[0, 7] == features[1, 7] == 3.0
    assert features[0, 4] == 10.0 and features[0, 5] == 0.0 and features[1, 4] == 0.0 and features[1, 5] == 10.0
    # a tie in float32 only: the distances differ in binary64, their float32 roundings do not, and the lower index still comes first
    both = lom.select(np.array([np.nextafter(9.0, INF), 9.0]), np.array([0, 0]), 2, 30.0)
    assert both == [0, 1]


def test_features_in_the_observers_frame(tables):
    _, lanes = tables['chain']
    f = see(lanes, 5, 3, psi=0.0)[0][0]                                      # heading along the lane, 3 m to its left
    assert f.tolist() == [0.0, -3.0, 0.0, 1.0, 5.0, 5.0, 3.0, 3.0]
    f = see(lanes, 5, 3, psi=math.pi)[0][0]                                  # against the lane: the foot is on the left, cos_rel = -1
    assert np.allclose(f, [0.0, 3.0, 0.0, -1.0, 5.0, 5.0, 3.0, 3.0], atol=1e-6) and f[3] < 0
    _, two = tables['dead_end']
    f = see(two, 2, 1, psi=0.0, md=INF)[0]
    assert f[0, 3] > 0 and f[1, 3] < 0                                       # its own lane, then the oncoming one


def test_polylines(tables):
    _, fork = tables['fork']
    _, points, n_valid, index = see(fork, 2, 0)                              # on lanelet 0 at arc 2: 2, 6 and 10 are on it, 14 is past the fork
    assert index[0] == 0 and n_valid[0] == 3 and points[0, :3].tolist() == [[0, 0], [4, 0], [8, 0]] and not points[0, 3:].any()
    assert set(index[1:3].tolist()) == {1, 2}                                # the branches are slots of their own
    _, chain = tables['chain']
    _, points, n_valid, index = see(chain, 2, 0, p=9)                        # through the unique successors to the dead end at 30 m
    assert index[0] == 0 and n_valid[0] == 8 and points[0, :8, 0].tolist() == [0, 4, 8, 12, 16, 20, 24, 28] and not points[0, :, 1].any()
    _, points, n_valid, index = see(chain, 2, 0, p=32, spacing=1.0)
    assert n_valid[0] == 29 and points[0, 28].tolist() == [28, 0]
    _, tagged = tables['tagged']
    assert see(tagged, 2, 0)[2][0] == 3                                      # the successor carries an excluded tag: the polyline ends
    _, points, n_valid, index = see(chain, 2, 1, p=1)                        # P = 1: the centre-line point at the foot
    assert points.shape == (4, 1, 2) and n_valid.tolist() == [1, 1, 1, 0] and points[0, 0].tolist() == [0, -1]


def test_the_hop_limit_ends_a_polyline_on_the_loop(tables):
    _, lanes = tables['loop']
    assert 12.3 < lanes.length(0) < 12.5 and 12.3 < lanes.length(1) < 12.5             # half circles of radius 4, in chords
    features, points, n_valid, index = see(lanes, 4, 0, psi=math.pi / 2, p=32, md=3.0)       # at the start of lanelet 0
    assert index[0] == 0 and features[0, 4] == 0.0
    # the start lanelet and MAX_HOPS more: 9 lengths of 12.42 m = 111.8 m, so the points at 0, 4, ..., 108 are valid: 28 of them
    reach = sum(lanes.length(l) for l in [0, 1] * 4 + [0])
    assert 108.0 < reach < 112.0 and n_valid[0] == 28 == int(reach // 4) + 1 and not points[0, 28:].any()
    assert lom.walk(lanes, 0, reach) is not None and lom.walk(lanes, 0, np.nextafter(reach, INF) + 1e-9) is None
