"""The float64 autograd model of differentiable time to collision (tests/ttc_grad_model.py; include/tdship.h "K9b") against central
differences of the forward model's lo (tests/ttc_model.py: pair_interval), on random pairs and on the slots of the random scenes the device tests
run; the numpy restatement of csrc/tds_ttc_grad.h against the autograd model; hand cases with exact answers; and the coverage the device tests
rely on.  CPU only."""
import numpy as np
import pytest
import torch

import ttc_grad_model as gm
import ttc_model as tm

F32, F64 = np.float32, np.float64
H = 1e-5                 # the step of the central differences
BOUND = 1e-6             # of max(1, |g|): the bar route_grad_model is held to against its differences
LEFT_OUT = 0.01          # the largest share of probes that may be left out because the binding axis moved
K, HORIZON, MARGIN = 4, 3.0, 0.25


def lo_and_axis(v, margin):
    """v (n, 14): ttc_model's lo of every pair, observer and other side by side, and the axis that binds there"""
    a, e = list(v[:, :7].T), list(v[:, 7:].T)
    _, lo, _ = tm.pair_interval(a, e, margin)
    return lo, gm.pair_choices(a, e, margin)['axis']


def hold_to_differences(label, a, e, margin):
    """every contributing pair of (a, e), 14 probes each -> the number of pairs; prints the figures before it asserts"""
    ok, t, ga, ge = gm.pair_gradients(a, e, margin)
    base = np.concatenate([np.stack(a, -1), np.stack(e, -1)], -1)[ok]
    g = np.concatenate([ga, ge], -1)[ok]
    lo, axis = lo_and_axis(base, margin)
    assert (np.abs(lo - t[ok]) <= 1e-12 * np.maximum(1.0, np.abs(lo))).all(), label                  # the torch branch IS the forward's lo
    probes = left_out = 0
    worst = 0.0
    for j in range(14):
        up, down = base.copy(), base.copy()
        up[:, j] += H
        down[:, j] -= H
        (lo_up, ax_up), (lo_down, ax_down) = lo_and_axis(up, margin), lo_and_axis(down, margin)
        keep = (ax_up == axis) & (ax_down == axis)
        probes += len(keep)
        left_out += int((~keep).sum())
        if keep.any():
            worst = max(worst, float((np.abs((lo_up - lo_down) / (2 * H) - g[:, j]) / np.maximum(1.0, np.abs(g[:, j])))[keep].max()))
    print(f'{label}: {int(ok.sum())} pairs with lo > 0, {probes} probes, {left_out} left out (binding axis moved), worst disagreement {worst:.3g} of max(1, |g|)')
    assert probes > 0 and left_out <= LEFT_OUT * probes
    assert worst <= BOUND
    return int(ok.sum())


def test_random_pairs_against_central_differences():
    a, e = gm.pairs_values(tm.random_pairs())
    lo = gm.pair_choices(a, e)['lo']
    within = (lo > 0) & (lo <= 5.0)
    assert within.sum() >= 100
    a, e = [v[within] for v in a], [v[within] for v in e]
    assert hold_to_differences('random pairs', a, e, 0.0) == within.sum()


def scene_slots(name):
    """the filled slots of a random scene at K = 4, horizon 3, margin 0.25 -> (a, e) values of the slots that may contribute, and the scene"""
    s, A = tm.scenes(name)
    ttc, index = tm.time_to_collision(s['boxes'], s['sc'], s['speed'], s['present'], A, K, HORIZON, MARGIN)
    V, b, a, k, e = gm.slots_of(s['boxes'], s['sc'], s['speed'], index)
    return list(V[b, a].T), list(V[b, e].T), (s, A, ttc, index, (b, a, k, e))


#: the positive slots the device tests rely on, at least
COVERAGE = {'E6': 7, 'E64': 15, 'E65': 13, 'E130': 17, 'mask40': 32}


@pytest.mark.parametrize('name', list(tm.SCENES))
def test_the_scenes_slots_against_central_differences(name):
    a, e, (s, A, ttc, index, (b, ai, k, ei)) = scene_slots(name)
    margin = float(F32(MARGIN))
    positive = hold_to_differences(name, a, e, margin)
    ok = gm.pair_choices(a, e, margin)['contributes']
    # a slot contributes exactly where the forward's time is above 0
    assert np.array_equal(ok, ttc[b, ai, k] > 0), name
    assert positive >= COVERAGE.get(name, 1), (name, positive)


def test_the_restatement_of_the_header_against_autograd():
    """float64 both, other orders of operations.  Every term of a partial is at most some 200 / |w| (metres and metres per second of these
    scenes), there are some 30 operations, and one of the 14 partials of a pair is at least 0.7 / |w| (|n| = 1): 1e-11 of the pair's largest
    partial is a hundred times that rounding"""
    sets = [gm.pairs_values(tm.random_pairs()) + [0.0]] + [list(scene_slots(name)[:2]) + [float(F32(MARGIN))] for name in tm.SCENES]
    contributing = 0
    for a, e, margin in sets:
        ok, t, ga, ge = gm.pair_gradients(a, e, margin)
        ok2, ra, re = gm.pair_partials(a, e, margin)
        assert np.array_equal(ok, ok2)
        scale = np.maximum(1.0, np.abs(np.concatenate([ga, ge], -1)).max(-1, keepdims=True))
        worst = max(float((np.abs(ra - ga) / scale).max()), float((np.abs(re - ge) / scale).max()))
        assert worst <= 1e-11, worst
        assert not ra[~ok].any() and not re[~ok].any()
        contributing += int(ok.sum())
    assert contributing >= 200


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------------
X, Y, LENGTH, WIDTH, SIN, COS, SPEED = range(7)


def one_slot(k):
    """definition_cases() scene 0, horizon 3, margin 0: a unit gradient on slot k of observer 0 -> (the entity, ga (7,), ge (7,)) from the autograd
    model, and the same from the restatement of the header"""
    c = tm.definition_cases()
    ttc, index = tm.time_to_collision(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, tm.DEFINITION_HORIZON, 0.0)
    assert index.tolist() == tm.DEFINITION_INDEX
    g = np.zeros(ttc.shape, F32)
    g[0, 0, k] = 1.0
    gb, gsc, gv, contributes = gm.scene_gradients(c['boxes'], c['sc'], c['speed'], index, g, 0.0)
    e = int(index[0, 0, k])
    assert contributes[0, 0, k] and not contributes[1].any()
    row = lambda j: np.array([gb[0, j, 0], gb[0, j, 1], gb[0, j, 2], gb[0, j, 3], gsc[0, j, 0], gsc[0, j, 1], gv[0, j]])
    assert not gb[1].any() and not gsc[1].any() and not gv[1].any() and not gb[..., 4].any()
    untouched = [j for j in range(6) if j not in (0, e)]
    assert not gb[0, untouched].any() and not gsc[0, untouched].any() and not gv[0, untouched].any()
    V = np.concatenate([c['boxes'][0, :, :4], c['sc'][0], c['speed'][0, :, None]], -1).astype(F64)
    ok, ra, re = gm.pair_partials([V[0:1, i] for i in range(7)], [V[e:e + 1, i] for i in range(7)], 0.0)
    assert ok[0]
    return e, row(0), row(e), ra[0], re[0]


@pytest.mark.parametrize('k, entity, t, observer, other', [
    (0, 1, 2.3, {X: -0.05, LENGTH: -0.025, SPEED: -0.115, COS: -1.25}, {X: 0.05, LENGTH: -0.025, SPEED: -0.115, COS: 1.25}),
    (1, 3, 2.3, {X: -0.1, LENGTH: -0.05, SPEED: -0.23}, {X: 0.1, WIDTH: -0.05, SPEED: 0.0}),
    (2, 4, 3.0, {X: -0.1, LENGTH: -0.05, SPEED: -0.3}, {X: 0.1, LENGTH: -0.05, SPEED: 0.3})])
def test_hand_cases(k, entity, t, observer, other):
    """head-on (axes 0 and 2 tie: axis 0 wins, which shows in the cos column), a crossing at right angles, a standing entity at the horizon"""
    e, ga, ge, ra, re = one_slot(k)
    assert e == entity
    for got_a, got_e in ((ga, ge), (ra, re)):
        for col, want in observer.items():
            assert abs(got_a[col] - want) <= 1e-12, (k, 'observer', gm.NAMES[col], got_a[col], want)
        for col, want in other.items():
            assert abs(got_e[col] - want) <= 1e-12, (k, 'other', gm.NAMES[col], got_e[col], want)
        assert got_a[Y] == 0 and got_e[Y] == 0


def test_slots_that_contribute_nothing():
    """the empty slot of observer 0, the overlapping pair of scene 1 (t = 0) and an index that is garbage: zero, whatever comes in"""
    c = tm.definition_cases()
    ttc, index = tm.time_to_collision(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, tm.DEFINITION_HORIZON, 0.0)
    g = np.where((ttc > 0) & np.isfinite(ttc), F32(1.0), F32(np.nan))      # a NaN comes in wherever the time is 0 or +inf
    index = index.copy()
    index[0, 2, :3] = [77, -5, 2]                   # out of range twice, and the observer itself
    gb, gsc, gv, contributes = gm.scene_gradients(c['boxes'], c['sc'], c['speed'], index, g, 0.0)
    assert not contributes[1].any() and not contributes[0, 2].any() and contributes[0, 0, :3].all()
    assert np.isfinite(gb).all() and np.isfinite(gsc).all() and np.isfinite(gv).all()
    assert not gb[1].any() and not gsc[1].any() and not gv[1].any()


def test_float32_model_is_close_to_float64():
    """the yardstick of the device tests exists and is small: the float32 run of the formula on a scene"""
    a, e, (s, A, ttc, index, _) = scene_slots('E64')
    g = np.random.default_rng(1).standard_normal(ttc.shape).astype(F32)
    g64 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], index, g, MARGIN)
    g32 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], index, g, MARGIN, torch.float32)
    assert np.array_equal(g64[3], g32[3])
    for x64, x32 in zip(g64[:3], g32[:3]):
        assert np.abs(x64).max() > 0 and np.abs(x64 - x32).max() <= 1e-3 * max(1.0, np.abs(x64).max())
