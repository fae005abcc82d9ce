"""CPU checks of the neighbour-observation model (tests/neighbors_model.py, binary32, what csrc/neighbors.hip must equal bit for bit) against an
independent float64 restatement of the definition (include/tdship.h "K6"), and the definition's edge cases by hand.

Features: |model - float64| <= 4 x the float32-against-float64 difference of a SEPARATE float32 evaluation of the formulas
(neighbors_model.features64 with dtype=float32), measured and printed here per feature on these very inputs -- and that yardstick is itself held
to what binary32 allows at these magnitudes.
Choice: right in float64 up to rounding.  Each of dx, dy, the two squares and the sum is rounded once, so the float32 d2 carries at most
4 * 2^-24 relative error; twice that is the margin: consecutive slots have d2_64[k + 1] >= d2_64[k] * (1 - eps) and every candidate left out has
d2_64 >= d2_64[last] * (1 - eps), eps = 8 * 2^-24."""
import numpy as np
import pytest

import neighbors_model as nm

EPS = 8 * 2.0 ** -24
FACTOR = 4


@pytest.mark.parametrize('seed,B,A,E,K,max_distance', [(1, 4, 6, 24, 8, 50.0), (2, 3, 5, 70, 32, 30.0), (3, 2, 9, 9, 4, float('inf')), (4, 2, 4, 130, 16, 45.0)])
def test_model_against_the_float64_restatement(seed, B, A, E, K, max_distance):
    s = nm.random_scenes(seed, B, A, E)
    features, index = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], A, K, max_distance)
    assert features.shape == (B, A, K, 8) and features.dtype == np.float32 and index.shape == (B, A, K) and index.dtype == np.int32
    r2 = float(np.float32(max_distance)) ** 2
    diff, yard, filled = np.zeros(8), np.zeros(8), 0
    for b in range(B):
        for a in range(A):
            who = index[b, a][index[b, a] >= 0]
            n = len(who)
            assert (index[b, a, n:] == -1).all() and (features[b, a, n:] == 0).all()            # the filled slots come first, empty ones are zero
            if not s['present'][b, a]:
                assert n == 0
                continue
            assert len(set(who)) == n and a not in who and s['present'][b, who].all()
            d2 = nm.d2_64(s['boxes'], b, a)
            assert (d2[who] <= r2 * (1 + EPS)).all()
            assert (d2[who][1:] >= d2[who][:-1] * (1 - EPS)).all()                                  # nearest first, up to rounding
            out = np.setdiff1d(np.nonzero(s['present'][b] & (np.arange(E) != a) & (d2 <= r2 * (1 - EPS)))[0], who)
            if len(out):                                                                             # candidates left out: the row is full and they are no nearer
                assert n == K and (d2[out] >= d2[who[-1]] * (1 - EPS)).all()
            f64 = nm.features64(s['boxes'], s['sc'], s['speed'], b, a, who)
            f32 = nm.features64(s['boxes'], s['sc'], s['speed'], b, a, who, dtype=np.float32)
            if n:
                diff = np.maximum(diff, np.abs(features[b, a, :n].astype(np.float64) - f64).max(0))
                yard = np.maximum(yard, np.abs(f32.astype(np.float64) - f64).max(0))
            filled += n
    print(f'seed {seed}: {filled} filled slots of {B * A * K}')
    for name, d, y in zip(('x', 'y', 'sin', 'cos', 'vx', 'vy', 'length', 'width'), diff, yard):
        print(f'  {name:6s} model against float64 {d:.3g}, float32 yardstick against float64 {y:.3g} (bound {FACTOR * y:.3g})')
    assert filled > B * A and (diff <= FACTOR * yard).all()
    # the yardstick is a float32 rounding figure: |dx|, |dy| <= 120 m (ulp 7.6e-6), three roundings each for x, y; sin, cos of the difference <= 1
    # (three roundings of 6e-8); velocities <= 15 m/s times that, two more roundings (ulp 9.5e-7); sizes are copied
    assert (yard[:2] <= 4e-5).all() and (yard[2:4] <= 4e-7).all() and (yard[4:6] <= 8e-6).all() and (yard[6:] == 0).all()


def test_the_definition_cases_by_hand():
    c = nm.definition_cases()
    features, index = nm.neighbors(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, nm.DEFINITION_MAX_DISTANCE)
    assert index.tolist() == nm.DEFINITION_INDEX
    assert (features[index < 0] == 0).all() and np.isfinite(features).all()
    # observer 0 of scene 0 heads along psi = 0.3: entity 1 at (3, 4) is ahead and to the left; its heading is -2.0, so -2.3 relative
    f = features[0, 0, 0].astype(np.float64)
    s, c0 = np.sin(0.3), np.cos(0.3)
    want = [3 * c0 + 4 * s, 4 * c0 - 3 * s, np.sin(-2.3), np.cos(-2.3), 3.0 * np.cos(-2.3) - 5.0, 3.0 * np.sin(-2.3), 4.0, 1.8]
    np.testing.assert_allclose(f, want, atol=2e-6)
    # the mirrored pair: the same bits of d2, so the lower index first, and y of opposite sign before the rotation
    assert index[0, 0, 0] == 1 and index[0, 0, 1] == 2
    # the coincident pair of scene 1 sees each other at (0, 0)
    assert (features[1, 1, 0, :2] == 0).all() and (features[1, 2, 0, :2] == 0).all()
    # a larger radius lets entity 4 in, behind entity 3 (d2 one step above)
    _, wider = nm.neighbors(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, 10.1)
    assert wider[0, 0].tolist() == [1, 2, 3, 4]
    # one slot: the nearest alone
    _, one = nm.neighbors(c['boxes'], c['sc'], c['speed'], c['present'], 3, 1, nm.DEFINITION_MAX_DISTANCE)
    assert one[..., 0].tolist() == [[1, 0, 0], [-1, 2, 1]]


def test_the_radius_is_inclusive_to_the_bit():
    """d2 == r2 is in, the next float32 above is out, whatever max_distance -- r2 is max_distance * max_distance rounded once"""
    for md in (10.0, 7.3, 0.0, 123.456):
        r2 = np.float32(md) * np.float32(md)
        boxes = np.zeros((1, 3, 5), np.float32)
        boxes[0, 1, 0] = np.float32(md)                                          # d2 = md * md: the same product
        boxes[0, 2, 1] = np.float32(md)
        s = dict(boxes=boxes, sc=nm.heading_sc(boxes[..., 4]), speed=np.zeros((1, 3), np.float32), present=np.ones((1, 3), bool))
        _, index = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], 1, 4, md)
        assert index[0, 0].tolist() == [1, 2, -1, -1], md
        assert boxes[0, 1, 0] * boxes[0, 1, 0] == r2
    _, index = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], 1, 4, float(np.nextafter(np.float32(123.456), np.float32(0))))
    assert index[0, 0].tolist() == [-1, -1, -1, -1]


def test_nan_poses_absent_entities_and_the_visible_mask():
    s = nm.random_scenes(11, 2, 4, 12, side=30.0, duplicates=0.0, absent=0.0)
    s['boxes'][0, 5, 0] = np.nan                                                     # a NaN neighbour
    s['boxes'][1, 1, 1] = np.nan                                                     # a NaN observer: every d2 is NaN, an empty row
    s['present'][0, 2] = False
    args = (s['boxes'], s['sc'], s['speed'], s['present'], 4, 11, float('inf'))
    features, index = nm.neighbors(*args)
    assert 5 not in index[0] and 2 not in index[0] and (index[0, 2] == -1).all() and (index[1, 1] == -1).all() and 1 not in index[1]
    assert (np.sort(index[0, 0])[2:] == [1, 3, 4, 6, 7, 8, 9, 10, 11]).all() and (index[0, 0, 9:] == -1).all()       # K larger than the candidates
    assert np.isfinite(features).all()
    g = np.random.default_rng(5)
    visible = g.random((2, 4, 12)) < 0.5
    fv, iv = nm.neighbors(*args, visible=visible)
    for b in range(2):
        for a in range(4):
            seen = [e for e in index[b, a] if e >= 0 and visible[b, a, e]]                  # the visible ones, in the same order
            assert iv[b, a].tolist() == seen + [-1] * (11 - len(seen))
    ones_f, ones_i = nm.neighbors(*args, visible=np.ones((2, 4, 12), np.uint8))
    assert np.array_equal(ones_i, index) and np.array_equal(ones_f, features)
    assert np.array_equal(nm.neighbors(*args, visible=visible.astype(np.uint8) * 7)[1], iv)    # any non-zero byte
