"""The float64 autograd model of the differentiable neighbour observations (tests/neighbors_grad_model.py; include/tdship.h "K6b")
against central differences of the forward model's features (tests/neighbors_model.py: features64) on the filled slots of the random scenes the
device tests run; hand cases with answers from the definition's table; and the coverage the device tests rely on.  CPU only."""
import numpy as np
import pytest
import torch

import neighbors_grad_model as gm
import neighbors_model as nm

F32, F64 = np.float32, np.float64
H = 1e-3                 # the step of the central differences
BOUND = 1e-6             # of max(1, |entry|)


@pytest.fixture(scope='module')
def scenes():
    """name -> (scene, A, K, index): the forward model's index of every case of the device tests"""
    out = {}
    for name, (seed, B, A, E, K, reach) in gm.CASES.items():
        s = nm.random_scenes(seed, B, A, E)
        out[name] = (s, A, K, nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], A, K, reach)[1])
    return out


def pair_scene(s, b, a, e):
    """the two entities of one slot as a scene of their own, float64: observer 0, entity 1"""
    pick = lambda v: np.stack([v[b, a], v[b, e]])[None].astype(F64)
    return pick(s['boxes']), pick(s['sc']), pick(s['speed'])


@pytest.mark.parametrize('name', list(gm.CASES))
def test_the_scenes_slots_against_central_differences(scenes, name):
    """Slot by slot, so that every one of a slot's 12 inputs is probed on its own: the slot is a scene of two entities, the loss its eight
    features times a random gradient.  The features are polynomials of degree at most 3 in the inputs and of degree 1 in each input alone, so a
    central difference along one input has no truncation error at all; what is left is rounding, some 1e-16 * 200 / h = 2e-11 of values of up to
    200 (metres times a gradient of order 1) at h = 1e-3.  The bound of 1e-6 of max(1, |entry|) lies far above both."""
    s, A, K, index = scenes[name]
    E = s['boxes'].shape[1]
    filled, b, a, k, e = gm.filled_slots(index, E)
    assert filled.sum() >= gm.FILLED[name]
    pick = np.random.default_rng(7).permutation(len(b))[:150]
    g = np.random.default_rng(len(name)).standard_normal((len(b), 8))
    worst = 0.0
    one = np.array([[[1]]], np.int32)
    for i in pick:
        boxes, sc, speed = pair_scene(s, b[i], a[i], e[i])
        assert np.isfinite(boxes[..., :4]).all()
        gb, gsc, gv, f = gm.scene_gradients(boxes, sc, speed, one, g[i][None, None, None].astype(F32))
        assert f.all()
        got = np.concatenate([gb[0, :, :4], gsc[0], gv[0, :, None]], -1)             # (2, 7)
        gi = g[i].astype(F32).astype(F64)
        loss = lambda bx, h, v: float((nm.features64(bx, h, v, 0, 0, np.array([1]))[0] * gi).sum())
        for ent in (0, 1):
            for col in range(7):
                args = []
                for sign in (1.0, -1.0):
                    bx, h, v = boxes.copy(), sc.copy(), speed.copy()
                    if col < 4:
                        bx[0, ent, col] += sign * H
                    elif col < 6:
                        h[0, ent, col - 4] += sign * H
                    else:
                        v[0, ent] += sign * H
                    args.append(loss(bx, h, v))
                diff = (args[0] - args[1]) / (2 * H)
                worst = max(worst, abs(diff - got[ent, col]) / max(1.0, abs(got[ent, col])))
    print(f'{name}: {int(filled.sum())} filled slots of {filled.size}, {len(pick)} probed on 14 inputs each, worst disagreement {worst:.3g} of max(1, |entry|)')
    assert worst <= BOUND


@pytest.mark.parametrize('name', list(gm.CASES))
def test_a_scene_is_the_sum_of_its_slots(scenes, name):
    """the scene-wide gradient is the slots' own gradients added at their two entities: float64 both, another order of the additions.  An entry
    is the sum of at most some hundred terms of at most some 200 g: 1e-10 of max(1, |entry|) is a hundred times that rounding"""
    s, A, K, index = scenes[name]
    B, E = s['boxes'].shape[:2]
    g = np.random.default_rng(3).standard_normal(index.shape + (8,)).astype(F32)
    gb, gsc, gv, filled = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], index, g)
    whole = np.concatenate([gb[..., :4], gsc, gv[..., None]], -1)
    _, b, a, k, e = gm.filled_slots(index, E)
    total = np.zeros((B, E, 7))
    n = len(b)
    pairs = [np.stack([v[b, a], v[b, e]], 1) for v in (s['boxes'], s['sc'], s['speed'])]
    pb, psc, pv, f = gm.scene_gradients(*pairs, np.ones((n, 1, 1), np.int32), g[b, a, k][:, None, None])
    per = np.concatenate([pb[..., :4], psc, pv[..., None]], -1)                       # (n, 2, 7)
    np.add.at(total, (b, a), per[:, 0])
    np.add.at(total, (b, e), per[:, 1])
    assert f.all() and np.abs(total - whole).max() <= 1e-10 * max(1.0, np.abs(whole).max())
    untouched = ~gm.touched(filled, index, E)
    assert not whole[untouched].any() and not gb[..., 4].any()
    print(f'{name}: {int(filled.sum())} filled, {int((~filled).sum())} empty, {int(untouched.sum())} entities no slot touches')


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------------
def by_the_table(c, b, a, e, f):
    """the definition's table for a unit gradient on feature f of a slot (observer a, entity e of scene b) in plain Python floats ->
    (entity's row, observer's row) as dicts"""
    g = [0.0] * 8
    g[f] = 1.0
    val = lambda t, *i: float(t[i])
    s, cs = val(c['sc'], b, a, 0), val(c['sc'], b, a, 1)
    se, ce = val(c['sc'], b, e, 0), val(c['sc'], b, e, 1)
    dx, dy = val(c['boxes'], b, e, 0) - val(c['boxes'], b, a, 0), val(c['boxes'], b, e, 1) - val(c['boxes'], b, a, 1)
    ve = val(c['speed'], b, e)
    f2, f3 = se * cs - ce * s, ce * cs + se * s
    G2, G3 = g[2] + g[5] * ve, g[3] + g[4] * ve
    px, py = g[0] * cs - g[1] * s, g[0] * s + g[1] * cs
    entity = dict(x=px, y=py, length=g[6], width=g[7], sin=G2 * cs + G3 * s, cos=-G2 * s + G3 * cs, speed=g[4] * f3 + g[5] * f2)
    observer = dict(x=-px, y=-py, length=0.0, width=0.0, sin=g[0] * dy - g[1] * dx - G2 * ce + G3 * se, cos=g[0] * dx + g[1] * dy + G2 * se + G3 * ce,
                    speed=-g[4])
    return entity, observer


#: (scene, observer, slot): the nearest of observer 0; the fourth slot of observer 1; an entity standing on its observer (dx = dy = 0)
HAND_SLOTS = [(0, 0, 0), (0, 0, 2), (0, 1, 3), (1, 1, 0)]


@pytest.mark.parametrize('slot', HAND_SLOTS)
@pytest.mark.parametrize('feature', range(8))
def test_hand_cases(slot, feature):
    c = nm.definition_cases()
    index = np.array(nm.DEFINITION_INDEX, np.int32)
    assert np.array_equal(nm.neighbors(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, nm.DEFINITION_MAX_DISTANCE)[1], index)
    b, a, k = slot
    e = int(index[b, a, k])
    assert e >= 0
    g = np.full(index.shape + (8,), np.nan, F32)                       # a NaN comes in at every empty slot
    g[index >= 0] = 0.0
    g[b, a, k, feature] = 1.0
    gb, gsc, gv, filled = gm.scene_gradients(c['boxes'], c['sc'], c['speed'], index, g)
    assert np.array_equal(filled, index >= 0)
    rows = np.concatenate([gb[..., :4], gsc, gv[..., None]], -1)
    entity, observer = by_the_table(c, b, a, e, feature)
    for j, want in ((e, entity), (a, observer)):
        for col, name in enumerate(gm.NAMES):
            assert abs(rows[b, j, col] - want[name]) <= 1e-14 * max(1.0, abs(want[name])), (slot, feature, j, name, rows[b, j, col], want[name])
    rows[b, [a, e]] = 0.0
    assert not rows.any() and not gb[..., 4].any(), 'the other rows are exactly 0'
    nonzero = {0: ('x', 'y'), 1: ('x', 'y'), 2: ('sin', 'cos'), 3: ('sin', 'cos'), 4: ('sin', 'cos', 'speed'), 5: ('sin', 'cos', 'speed'), 6: ('length',),
               7: ('width',)}[feature]
    assert {n for n, v in entity.items() if v != 0} <= set(nonzero) and any(entity[n] != 0 for n in nonzero)


def test_slots_that_contribute_nothing():
    """an empty slot and an index that is garbage: zero, whatever comes in"""
    c = nm.definition_cases()
    index = np.array(nm.DEFINITION_INDEX, np.int32)
    index[0, 2, :3] = [77, -5, 2]                   # out of range twice, and the observer itself
    filled = gm.filled_slots(index, 5)[0]
    assert filled[0, 0, :3].all() and not filled[0, 2].any() and not filled[0, 0, 3] and not filled[1, 0].any()
    g = np.where(filled[..., None], F32(1.0), F32(np.nan))
    gb, gsc, gv, again = gm.scene_gradients(c['boxes'], c['sc'], c['speed'], index, g)
    assert np.array_equal(again, filled)
    assert np.isfinite(gb).all() and np.isfinite(gsc).all() and np.isfinite(gv).all()
    untouched = ~gm.touched(filled, index, 5)
    assert untouched[1, 0] and untouched[1, 3] and untouched[1, 4] and not untouched[0, :4].any()
    assert not gb[untouched].any() and not gsc[untouched].any() and not gv[untouched].any() and gb[0, [1, 2, 3]].any(-1).all()


def test_float32_model_is_close_to_float64(scenes):
    """the yardstick of the device tests exists and is small: the float32 run of the formula on a scene"""
    s, A, K, index = scenes['E64']
    g = np.random.default_rng(1).standard_normal(index.shape + (8,)).astype(F32)
    g64 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], index, g)
    g32 = gm.scene_gradients(s['boxes'], s['sc'], s['speed'], index, g, torch.float32)
    assert np.array_equal(g64[3], g32[3])
    for x64, x32 in zip(g64[:3], g32[:3]):
        yard, largest = np.abs(x64 - x32).max(), np.abs(x64).max()
        print(f'float32 model against float64 {yard:.3g}, largest entry {largest:.3g}')
        assert largest > 0 and 0 < yard <= 1e-5 * max(1.0, largest)
        assert 0.5 * float(np.spacing(F32(largest))) <= 4 * yard, 'half a binary32 ulp of the largest entry lies inside the device tests\' bar'
