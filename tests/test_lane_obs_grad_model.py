"""The float64 autograd model of the differentiable lane observations (tests/lane_obs_grad_model.py; include/tdship.h "K8b")
against central differences of the forward model (tests/lane_obs_model.py, through `observe64`: the same functions without the rounding of the
outputs to float32, held here to `observe` bit for bit) on the synthetic maps; hand cases with exact answers; slots and points that contribute
nothing.  CPU only."""
import math

import numpy as np
import pytest
import torch

import lane_obs_cases as cases
import lane_obs_grad_model as gm
import lane_obs_model as lom

F32, F64 = np.float32, np.float64
H = 1e-5                 # the step of the central differences
BOUND = 1e-6             # of max(1, |g|): the bars of tests/test_ttc_grad_model.py
LEFT_OUT = 0.01          # the largest share of probes that may be left out because a discrete choice moved
K, P, SPACING, REACH = 4, 5, 4.0, 12.0
MAPS = dict(cases.STRUCTURES, ring=cases.ring)


@pytest.fixture(scope='module')
def tables():
    return {name: lom.Lanes(make()) for name, make in MAPS.items()}


def random_poses(name, n=40):
    """(n - 2, 4) float32 [x, y, sin, cos]: lane_obs_cases.poses without its first two, which sit exactly on centre-line points (kinks)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    p = cases.poses(rng, MAPS[name](), n)[2:]
    return np.stack([p[:, 0], p[:, 1], np.sin(p[:, 2]), np.cos(p[:, 2])], -1).astype(F32)


def test_observe64_rounds_to_the_forward_model(tables):
    """the function the differences are taken of IS lane_obs_model.observe before its rounding: features, points and index, every bit"""
    slots = 0
    for name, lanes in tables.items():
        for pose in random_poses(name, 12):
            f, p, index, _ = gm.observe64(lanes, pose.astype(F64), K, P, SPACING, REACH)
            want = lom.observe(lanes, pose, True, K, P, SPACING, REACH)
            assert np.array_equal(f.astype(F32).view(np.int32), want[0].view(np.int32)) and np.array_equal(index, want[3]), name
            assert np.array_equal(p.astype(F32).view(np.int32), want[1].view(np.int32)), name
            slots += int((index >= 0).sum())
    assert slots >= 100


def test_against_central_differences(tables):
    """a random gradient on every feature and point; the four inputs x, y, sin, cos of every pose one at a time.  A probe whose discrete choices
    (lanelets and their order, sb, the clamp, every point's lanelet, segment and validity) differ between -H and +H is left out"""
    probes = left_out = filled = points = 0
    worst = 0.0
    for name, lanes in tables.items():
        rng = np.random.default_rng(len(name))
        for pose in random_poses(name):
            base = pose.astype(F64)
            f0, p0, index, key = gm.observe64(lanes, base, K, P, SPACING, REACH)
            if not (index >= 0).any():
                continue
            gf, gp = rng.standard_normal((K, 8)).astype(F32), rng.standard_normal((K, P, 2)).astype(F32)
            g_xy, g_sc, fil, val = gm.gradients([lanes], pose[None, None, :2], pose[None, None, 2:], index[None, None].astype(np.int32), gf[None, None],
                                                gp[None, None], P, SPACING)
            assert np.array_equal(fil[0, 0], index >= 0)
            filled, points = filled + int(fil.sum()), points + int(val.sum())
            g = np.concatenate([g_xy[0, 0], g_sc[0, 0]])
            for i in range(4):
                up, down = base.copy(), base.copy()
                up[i] += H
                down[i] -= H
                fu, pu, _, ku = gm.observe64(lanes, up, K, P, SPACING, REACH)
                fd, pd, _, kd = gm.observe64(lanes, down, K, P, SPACING, REACH)
                probes += 1
                if ku != key or kd != key:
                    left_out += 1
                    continue
                diff = (((fu - fd) * gf.astype(F64)).sum() + ((pu - pd) * gp.astype(F64)).sum()) / (2 * H)
                worst = max(worst, abs(diff - g[i]) / max(1.0, abs(g[i])))
    print(f'lane observations: {probes} probes on {filled} filled slots and {points} valid points, {left_out} left out (a discrete choice moved), '
          f'worst disagreement {worst:.3g} of max(1, |g|)')
    assert probes >= 500 and filled >= 300 and points > filled and left_out <= LEFT_OUT * probes
    assert worst <= BOUND


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------------
ARC, LATERAL, DISTANCE = 4, 6, 7


def beside_the_chain(tables, x, y, feature=None, point=None, k=1, n_points=3):
    """an agent at (x, y, psi = 0) on `chain()`: a unit gradient on one feature of slot 0, or on one coordinate of one of its points -> (g_xy, g_sc)"""
    lanes = tables['chain']
    pose = np.array([x, y, 0.0, 1.0], F32)
    index = lom.observe(lanes, pose, True, k, n_points, SPACING, REACH)[3]
    assert index[0] == 0
    gf, gp = np.zeros((1, 1, k, 8), F32), np.zeros((1, 1, k, n_points, 2), F32)
    if feature is not None:
        gf[0, 0, 0, feature] = 1.0
    if point is not None:
        gp[0, 0, 0, point[0], point[1]] = 1.0
    g_xy, g_sc, filled, valid = gm.gradients([lanes], pose[None, None, :2], pose[None, None, 2:], index[None, None], gf, gp, n_points, SPACING)
    assert filled[0, 0, 0] and valid[0, 0, 0].all()
    return g_xy[0, 0], g_sc[0, 0]


def near(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() <= 1e-12


def test_beside_a_straight_lane(tables):
    """(4, 1) beside lanelet 0 of the chain, the foot inside a segment: lateral and distance grow with y, the arc with x, and the polyline
    slides along with the agent -- its points stay where they are ahead of it, and come nearer sideways as it moves away.
    (The centre line the library makes of chain() has a point at (5, 0), so x = 5 is a kink, not the inside of a segment: see the next test.)"""
    assert near(beside_the_chain(tables, 4.0, 1.0, feature=LATERAL)[0], (0.0, 1.0))
    assert near(beside_the_chain(tables, 4.0, 1.0, feature=ARC)[0], (1.0, 0.0))
    assert near(beside_the_chain(tables, 4.0, 1.0, feature=DISTANCE)[0], (0.0, 1.0))
    for j in range(3):                                           # point 2 lies on the next lanelet: the slide reaches it all the same
        assert near(beside_the_chain(tables, 4.0, 1.0, point=(j, 0))[0], (0.0, 0.0)), 'the slide cancels the -I term'
        assert near(beside_the_chain(tables, 4.0, 1.0, point=(j, 1))[0], (0.0, -1.0))


def test_beside_a_centre_line_point_the_definition_takes_the_clamped_side(tables):
    """(5, 1) is level with the centre-line point (5, 0): sb = 0, the earlier of the two segments that share the foot, where u = 1 exactly -- not
    strictly inside (0, 1), so m = 0: no arc gradient and no slide, as at any clamped foot.  lateral and distance do not depend on m"""
    lanes = tables['chain']
    ch = gm.choices(lanes, np.array([5.0, 1.0, 0.0, 1.0], F32), [0], 3, SPACING)[0]
    assert ch['sb'] == 0 and ch['u'] == 1.0 and not ch['m']
    assert near(beside_the_chain(tables, 5.0, 1.0, feature=ARC)[0], (0.0, 0.0))
    assert near(beside_the_chain(tables, 5.0, 1.0, feature=LATERAL)[0], (0.0, 1.0))
    assert near(beside_the_chain(tables, 5.0, 1.0, feature=DISTANCE)[0], (0.0, 1.0))
    assert near(beside_the_chain(tables, 5.0, 1.0, point=(1, 0))[0], (-1.0, 0.0))


def test_behind_the_start_the_foot_is_clamped(tables):
    """(-2, 1): the foot is the lanelet's first point and stays there: no arc gradient, and the polyline does not slide"""
    assert near(beside_the_chain(tables, -2.0, 1.0, feature=ARC)[0], (0.0, 0.0))
    for j in range(3):
        assert near(beside_the_chain(tables, -2.0, 1.0, point=(j, 0))[0], (-1.0, 0.0))
        assert near(beside_the_chain(tables, -2.0, 1.0, point=(j, 1))[0], (0.0, -1.0))


def test_on_the_centre_line_distance_contributes_exactly_zero(tables):
    g_xy, g_sc = beside_the_chain(tables, 5.0, 0.0, feature=DISTANCE)
    assert not g_xy.any() and not g_sc.any()
    lanes = tables['chain']
    pose = np.array([5.0, 0.0, 0.0, 1.0], F32)
    index = lom.observe(lanes, pose, True, 3, 4, SPACING, REACH)[3]
    rng = np.random.default_rng(3)
    gf, gp = rng.standard_normal((1, 1, 3, 8)).astype(F32), rng.standard_normal((1, 1, 3, 4, 2)).astype(F32)
    with_distance = gm.gradients([lanes], pose[None, None, :2], pose[None, None, 2:], index[None, None], gf, gp, 4, SPACING)
    gf[..., 0, DISTANCE] = 0.0                                   # slot 0 is the lanelet the agent stands on
    without = gm.gradients([lanes], pose[None, None, :2], pose[None, None, 2:], index[None, None], gf, gp, 4, SPACING)
    for a, b in zip(with_distance[:2], without[:2]):
        assert np.isfinite(a).all() and np.array_equal(a, b) and a.any()


def test_a_nan_at_an_empty_slot_or_an_invalid_point_changes_nothing(tables):
    """the fork: the polyline of lanelet 0 ends at its end; k = 4 leaves an empty slot; garbage in the index is an empty slot too"""
    lanes = tables['fork']
    pose = np.array([2.0, 0.5, math.sin(0.3), math.cos(0.3)], F32)
    _, _, n_valid, index = lom.observe(lanes, pose, True, 4, 6, SPACING, REACH)
    assert index[3] == -1 and 0 < n_valid[0] < 6
    index = index.copy()
    index[2] = 77                                                # out of range: treated as empty
    rng = np.random.default_rng(4)
    gf, gp = rng.standard_normal((1, 1, 4, 8)).astype(F32), rng.standard_normal((1, 1, 4, 6, 2)).astype(F32)
    args = ([lanes], pose[None, None, :2], pose[None, None, 2:], index[None, None])
    clean = gm.gradients(*args, gf, gp, 6, SPACING)
    assert clean[2][0, 0].tolist() == [True, True, False, False] and not clean[3][0, 0, 2:].any()
    assert np.array_equal(clean[3][0, 0, :2], np.arange(6)[None] < n_valid[:2, None])
    gf[0, 0, 2:], gp[0, 0, 2:] = np.nan, np.inf
    gp[0, 0][~clean[3][0, 0]] = np.nan
    dirty = gm.gradients(*args, gf, gp, 6, SPACING)
    for a, b in zip(clean[:2], dirty[:2]):
        assert np.isfinite(b).all() and np.array_equal(a, b) and a.any()
    # no map, a NaN pose: nothing is filled
    assert not gm.gradients([None], *args[1:], gf, gp, 6, SPACING)[2].any()
    nan_pose = np.array([np.nan, 0.5, 0.0, 1.0], F32)
    out = gm.gradients([lanes], nan_pose[None, None, :2], nan_pose[None, None, 2:], index[None, None], gf, gp, 6, SPACING)
    assert not out[2].any() and not out[0].any() and not out[1].any()


def test_one_incoming_gradient_alone_and_the_float32_mode(tables):
    """None reads as zeros; the yardstick of the device tests exists and is small: the float32 run of the formula on the same choices"""
    lanes = tables['dead_end']
    poses = random_poses('dead_end', 10)
    xy, sc = poses[None, :, :2], poses[None, :, 2:]
    index = np.stack([lom.observe(lanes, p, True, K, P, SPACING, REACH)[3] for p in poses])[None]
    rng = np.random.default_rng(5)
    gf, gp = rng.standard_normal((1, 8, K, 8)).astype(F32), rng.standard_normal((1, 8, K, P, 2)).astype(F32)
    both = gm.gradients([lanes], xy, sc, index, gf, gp, P, SPACING)
    f_only, p_only = gm.gradients([lanes], xy, sc, index, gf, None, P, SPACING), gm.gradients([lanes], xy, sc, index, None, gp, P, SPACING)
    zeros = gm.gradients([lanes], xy, sc, index, gf, np.zeros_like(gp), P, SPACING)
    f32 = gm.gradients([lanes], xy, sc, index, gf, gp, P, SPACING, torch.float32)
    for i in range(2):
        assert np.array_equal(f_only[i], zeros[i]) and np.abs(f_only[i] + p_only[i] - both[i]).max() <= 1e-12 * np.abs(both[i]).max()
        assert np.abs(both[i]).max() > 0 and 0 < np.abs(both[i] - f32[i]).max() <= 1e-4 * max(1.0, np.abs(both[i]).max())
    assert np.array_equal(both[2], f32[2]) and np.array_equal(both[3], f32[3]) and both[2].sum() >= 8


def test_a_distance_that_is_zero_in_float32_alone_gives_no_nan(tables):
    """(4, 1e-30): d2 = 1e-60 is above 0 in float64 and rounds to 0 in float32, where the yardstick must stay finite -- the rule of distance == 0
    holds in the arithmetic that meets it"""
    lanes = tables['chain']
    pose = np.array([4.0, 1e-30, 0.0, 1.0], F32)
    index = lom.observe(lanes, pose, True, 2, 3, SPACING, REACH)[3]
    gf, gp = np.ones((1, 1, 2, 8), F32), np.ones((1, 1, 2, 3, 2), F32)
    for dtype in (torch.float64, torch.float32):
        g_xy, g_sc, filled, _ = gm.gradients([lanes], pose[None, None, :2], pose[None, None, 2:], index[None, None], gf, gp, 3, SPACING, dtype)
        assert filled[0, 0].all() and np.isfinite(g_xy).all() and np.isfinite(g_sc).all() and g_xy.any()
