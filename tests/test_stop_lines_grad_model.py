"""The float64 autograd model of the differentiable stop-line observations (tests/stop_lines_grad_model.py; include/tdship.h "K7b")
against central differences of the forward model's arithmetic (tests/lights_model.py: stop_lines, restated here in float64 as `features64`) on
random scenes and on the definition cases; hand cases with answers from the definition's table; and what the device tests rely on.  CPU only."""
import numpy as np
import pytest
import torch

import lights_model as lm
import stop_lines_grad_model as gm

F32, F64 = np.float32, np.float64
H = 1e-4                 # the step of the central differences
BOUND = 1e-6             # of max(1, |entry|): the bar of the other models
LEFT_OUT_CAP = 0.01      # the share of probes that may be left out because the step changes a slot's index

#: name -> (seed, B, A, N, K, max_distance, ahead_only, min_cos).  Observer 0 of every scene of lights_model.random_scenes stands exactly ON a line:
#: with ahead_only it sits on the filter's boundary x = 0, and a step along x or y moves the line out of its row -- the probes that are left out
SCENES = {'N6': (1, 1, 120, 6, 4, 80.0, True, None), 'N33': (2, 1, 120, 33, 4, 60.0, True, None), 'N65 both filters off': (3, 2, 60, 65, 8, 40.0, False, None),
          'N65 min_cos': (4, 1, 120, 65, 4, 60.0, True, 0.2), 'N200 K32': (5, 1, 20, 200, 32, float('inf'), False, None)}


def features64(xy, sc, lines, line_sc, ttc, index):
    """lights_model.stop_lines' arithmetic for ONE observer in float64, the slots' lines given: xy (2,), sc (2,), lines (N,5), line_sc (N,2),
    ttc (N,), index (K,) -> (K,8), zeros in the slots that are not filled"""
    out = np.zeros((len(index), 8))
    s, c = sc
    for k, n in enumerate(index):
        if not 0 <= n < len(lines):
            continue
        dx, dy = lines[n, 0] - xy[0], lines[n, 1] - xy[1]
        sl, cl = line_sc[n]
        out[k] = [dx * c + dy * s, dy * c - dx * s, sl * c - cl * s, cl * c + sl * s, lines[n, 2], lines[n, 3], ttc[n], np.sqrt(dx * dx + dy * dy)]
    return out


def forward_index(s, b, a, xy, sc, K, reach, ahead_only, min_cos):
    """the forward model's index of one observer at a pose of its own"""
    return lm.stop_lines(xy[None, None].astype(F32), sc[None, None].astype(F32), np.ones((1, 1), bool), s['lines'][b:b + 1], s['line_sc'][b:b + 1],
                         s['mask'][b:b + 1], s['state'][b:b + 1], s['time_to_change'][b:b + 1], K, reach, ahead_only=ahead_only, min_cos=min_cos)[1][0, 0]


def probe(s, K, reach, ahead_only, min_cos, rng, limit=10 ** 6):
    """-> (probes made, probes left out, worst disagreement): every present observer with a filled slot, each of its four inputs on its own"""
    index = lm.stop_lines(**s, k=K, max_distance=reach, ahead_only=ahead_only, min_cos=min_cos)[1]
    B, A = index.shape[:2]
    g = rng.standard_normal(index.shape + (8,)).astype(F32)
    g_xy, g_sc, filled = gm.scene_gradients(s['agent_xy'], s['agent_sc'], s['lines'], s['line_sc'], index, g, time_to_change=s['time_to_change'])
    got = np.concatenate([g_xy, g_sc], -1)
    made = left_out = 0
    worst = 0.0
    rows = np.argwhere(gm.observers(filled))
    for b, a in rows[rng.permutation(len(rows))[:limit]]:
        lines, line_sc, ttc = s['lines'][b].astype(F64), s['line_sc'][b].astype(F64), s['time_to_change'][b].astype(F64)
        gi = g[b, a].astype(F64)
        base = np.concatenate([s['agent_xy'][b, a], s['agent_sc'][b, a]]).astype(F64)
        for col in range(4):
            values, same = [], True
            for sign in (1.0, -1.0):
                v = base.copy()
                v[col] += sign * H
                same = same and np.array_equal(forward_index(s, b, a, v[:2], v[2:], K, reach, ahead_only, min_cos), index[b, a])
                values.append(float((features64(v[:2], v[2:], lines, line_sc, ttc, index[b, a]) * gi).sum()))
            made += 1
            if not same:
                left_out += 1
                continue
            diff = (values[0] - values[1]) / (2 * H)
            worst = max(worst, abs(diff - got[b, a, col]) / max(1.0, abs(got[b, a, col])))
    return made, left_out, worst


def test_random_scenes_against_central_differences():
    """x, y and the distance are the features that bend: the distance r has a third derivative of at most 3 / r^2, so a central difference at
    h = 1e-4 is off by at most h^2 / 2 r^2 = 5e-9 / r^2 -- below the bar for every r above 0.1 m; rounding adds some 1e-16 * 1e3 / h = 1e-9.
    An observer exactly on a line is probed too: r is even in the step there, the difference is exactly 0, and so is the definition's
    convention.  A probe is left out only where the step changes the forward model's index of that observer; the share of them is capped over
    all scenes together."""
    made = left_out = 0
    worst = 0.0
    for name, (seed, B, A, N, K, reach, ahead_only, min_cos) in SCENES.items():
        s = lm.random_scenes(seed, B, A, N)
        m, o, w = probe(s, K, reach, ahead_only, min_cos, np.random.default_rng(seed))
        print(f'{name}: {m} probes, {o} left out (the step changes a slot), worst disagreement {w:.3g} of max(1, |entry|)')
        assert m >= 40
        made, left_out, worst = made + m, left_out + o, max(worst, w)
    print(f'all scenes: {made} probes, {left_out} left out = {left_out / made:.2%} (cap {LEFT_OUT_CAP:.0%}), worst disagreement {worst:.3g} (bound {BOUND:g})')
    assert made >= 1500 and left_out <= LEFT_OUT_CAP * made and worst <= BOUND


@pytest.mark.parametrize('filters', list(lm.DEFINITION_INDEX))
def test_the_definition_cases_against_central_differences(filters):
    """the cases sit ON the boundaries of the filters (d2 = r2 exactly, x = 0 exactly), where a step does change the index: they are probed with
    the index held, which is what a constant of differentiation means, and the count of probes whose index would move is printed"""
    ahead_only, min_cos = filters
    c = lm.definition_cases()
    index = np.array(lm.DEFINITION_INDEX[filters], np.int32)
    assert np.array_equal(lm.stop_lines(**c, k=4, max_distance=lm.DEFINITION_MAX_DISTANCE, ahead_only=ahead_only, min_cos=min_cos)[1], index)
    g = np.random.default_rng(4).standard_normal(index.shape + (8,)).astype(F32)
    g[index < 0] = np.nan
    g_xy, g_sc, filled = gm.scene_gradients(c['agent_xy'], c['agent_sc'], c['lines'], c['line_sc'], index, g, time_to_change=c['time_to_change'])
    assert np.array_equal(filled, index >= 0) and np.isfinite(g_xy).all() and np.isfinite(g_sc).all()
    got = np.concatenate([g_xy, g_sc], -1)
    worst, moved, made = 0.0, 0, 0
    for b, a in np.argwhere(filled.any(-1)):
        lines, line_sc, ttc = c['lines'][b].astype(F64), c['line_sc'][b].astype(F64), c['time_to_change'][b].astype(F64)
        gi = np.where(filled[b, a][:, None], g[b, a].astype(F64), 0.0)
        base = np.concatenate([c['agent_xy'][b, a], c['agent_sc'][b, a]]).astype(F64)
        for col in range(4):
            values = []
            for sign in (1.0, -1.0):
                v = base.copy()
                v[col] += sign * H
                moved += not np.array_equal(forward_index(c, b, a, v[:2], v[2:], 4, lm.DEFINITION_MAX_DISTANCE, ahead_only, min_cos), index[b, a])
                values.append(float(np.nansum(features64(v[:2], v[2:], lines, line_sc, ttc, index[b, a]) * gi)))
            made += 1
            worst = max(worst, abs((values[0] - values[1]) / (2 * H) - got[b, a, col]) / max(1.0, abs(got[b, a, col])))
    print(f'definition cases {filters}: {made} probes with the index held ({moved} steps would move it), worst disagreement {worst:.3g}')
    assert made >= 12 and worst <= BOUND
    assert not got[~filled.any(-1)].any(), 'absent observers, NaN poses and rows without a line: exactly 0'


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------------
def by_the_table(c, b, a, n, g):
    """the definition's table in plain Python floats -> [to x, to y, to s, to c]"""
    val = lambda t, *i: float(t[i])
    s, cs = val(c['agent_sc'], b, a, 0), val(c['agent_sc'], b, a, 1)
    sl, cl = val(c['line_sc'], b, n, 0), val(c['line_sc'], b, n, 1)
    dx, dy = val(c['lines'], b, n, 0) - val(c['agent_xy'], b, a, 0), val(c['lines'], b, n, 1) - val(c['agent_xy'], b, a, 1)
    r = (dx * dx + dy * dy) ** 0.5
    q = 0.0 if r == 0 else g[7] / r
    return [-(g[0] * cs - g[1] * s) - q * dx, -(g[0] * s + g[1] * cs) - q * dy, g[0] * dy - g[1] * dx - g[2] * cl + g[3] * sl,
            g[0] * dx + g[1] * dy + g[2] * sl + g[3] * cl]


#: (scene, observer, slot) of DEFINITION_INDEX[(True, None)]: a 3-4-5 line, its mirror image turned by pi, and the observer standing ON a line
HAND_SLOTS = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 2, 0)]


@pytest.mark.parametrize('slot', HAND_SLOTS)
@pytest.mark.parametrize('feature', range(8))
def test_hand_cases(slot, feature):
    c = lm.definition_cases()
    index = np.array(lm.DEFINITION_INDEX[(True, None)], np.int32)
    b, a, k = slot
    n = int(index[b, a, k])
    assert n >= 0
    g = np.full(index.shape + (8,), np.nan, F32)                       # a NaN comes in at every empty slot
    g[index >= 0] = 0.0
    g[b, a, k, feature] = 1.0
    g_xy, g_sc, filled = gm.scene_gradients(c['agent_xy'], c['agent_sc'], c['lines'], c['line_sc'], index, g)
    rows = np.concatenate([g_xy, g_sc], -1)
    want = by_the_table(c, b, a, n, g[b, a, k].astype(F64))
    for col in range(4):
        assert abs(rows[b, a, col] - want[col]) <= 1e-14 * max(1.0, abs(want[col])), (slot, feature, col, rows[b, a, col], want[col])
    rows[b, a] = 0.0
    assert not rows.any(), 'the other rows are exactly 0'
    if feature in (4, 5, 6):
        assert not any(want), 'length, width and time_to_change send no gradient'
    if slot == (1, 0, 0):
        assert all(np.isfinite(want)) and (feature != 7 or not any(want)), 'on the line: the distance contributes exactly 0'
    elif feature in (0, 1, 7):
        assert any(want[:2])


def test_slots_that_contribute_nothing():
    """an empty slot and an index that is garbage: zero, whatever comes in; NaN at g4 .. g6 of a filled slot meets constants"""
    c = lm.definition_cases()
    index = np.array(lm.DEFINITION_INDEX[(True, None)], np.int32)
    index[0, 2, :3] = [77, -5, 6]
    filled = gm.filled_slots(index, 6)[0]
    assert filled[0, 0, :3].all() and not filled[0, 2].any() and not filled[0, 0, 3]
    g = np.where(np.broadcast_to(filled[..., None], filled.shape + (8,)), F32(1.0), F32(np.nan)).astype(F32)
    g[filled, 4:7] = np.nan
    g_xy, g_sc, again = gm.scene_gradients(c['agent_xy'], c['agent_sc'], c['lines'], c['line_sc'], index, g)
    assert np.array_equal(again, filled) and np.isfinite(g_xy).all() and np.isfinite(g_sc).all()
    assert not g_xy[~filled.any(-1)].any() and not g_sc[~filled.any(-1)].any() and g_xy[0, 0].any() and g_sc[0, 0].any()


def test_float32_model_is_close_to_float64():
    """the yardstick of the device tests exists and is small: the float32 run of the formula on a scene"""
    s = lm.random_scenes(2, 2, 17, 33)
    index = lm.stop_lines(**s, k=4, max_distance=60.0)[1]
    g = np.random.default_rng(1).standard_normal(index.shape + (8,)).astype(F32)
    g64 = gm.scene_gradients(s['agent_xy'], s['agent_sc'], s['lines'], s['line_sc'], index, g)
    g32 = gm.scene_gradients(s['agent_xy'], s['agent_sc'], s['lines'], s['line_sc'], index, g, torch.float32)
    assert np.array_equal(g64[2], g32[2])
    for x64, x32 in zip(g64[:2], g32[:2]):
        yard, largest = np.abs(x64 - x32).max(), np.abs(x64).max()
        print(f'float32 model against float64 {yard:.3g}, largest entry {largest:.3g}')
        assert largest > 0 and 0 < yard <= 1e-5 * max(1.0, largest)
        assert 0.5 * float(np.spacing(F32(largest))) <= 4 * yard, 'half a binary32 ulp of the largest entry lies inside the device tests\' bar'
