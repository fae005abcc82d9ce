"""The numpy model of time to collision (tests/ttc_model.py, the definition of include/tdship.h "K9") against a yardstick that shares nothing
with it -- rectangle overlap tested at fixed time steps --, on hand cases with exact answers, and the coverage of the random scenes the device
tests compare bit for bit.  CPU only."""
import numpy as np
import pytest

import ttc_model as tm

F32, F64 = np.float32, np.float64
INF = float('inf')
HORIZON, STEP = 5.0, 0.01


def interval_of(pairs):
    """pairs (n, 2, 6) float32 [x, y, l, w, psi, v] -> possible, lo, hi of the definition, [sin, cos] rounded to float32 as the kernel gets them"""
    sc = tm.nm.heading_sc(pairs[..., 4]).astype(F64)
    q = pairs.astype(F64)
    out = [tm.pair_interval([q[i, 0, 0], q[i, 0, 1], q[i, 0, 2], q[i, 0, 3], sc[i, 0, 0], sc[i, 0, 1], q[i, 0, 5]],
                            [q[i, 1:, 0], q[i, 1:, 1], q[i, 1:, 2], q[i, 1:, 3], sc[i, 1:, 0], sc[i, 1:, 1], q[i, 1:, 5]]) for i in range(len(q))]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def test_the_model_against_time_stepped_overlap():
    """4 000 random pairs in a 60 m square, speeds 0 .. 15 m/s, horizon 5 s, step 0.01 s: the verdicts agree and the times lie within a step.
    Left out: contacts shorter than two steps (a step may jump over them) and first contacts within a step of the horizon -- at most 5 % of the
    colliding pairs"""
    pairs = tm.random_pairs()
    possible, lo, hi = interval_of(pairs)
    collide = possible & (lo <= hi) & (hi >= 0)
    cand = collide & (lo <= HORIZON)
    t = np.where(cand, np.where(lo > 0, lo, 0.0), np.inf)
    left_out = collide & ((hi - np.maximum(lo, 0.0) < 2 * STEP) | (np.abs(lo - HORIZON) <= STEP))
    stepped = tm.stepped(pairs, HORIZON, STEP)
    print(f'{int(cand.sum())} of {len(pairs)} pairs collide within {HORIZON} s, {int((cand & (lo <= 0)).sum())} of them overlap already; '
          f'{int(collide.sum())} collide at some time, {int(left_out.sum())} of them left out')
    assert cand.sum() >= 100 and (cand & (lo <= 0)).sum() >= 20
    assert left_out.sum() <= 0.05 * collide.sum()
    keep = ~left_out
    assert np.array_equal(np.isfinite(t)[keep], np.isfinite(stepped)[keep]), np.argwhere((np.isfinite(t) != np.isfinite(stepped)) & keep)[:8].tolist()
    both = keep & np.isfinite(t)
    diff = np.abs(t[both] - stepped[both])
    print(f'largest difference to the stepped time {diff.max():.6f} s')
    assert (diff <= STEP + 1e-9).all()
    # the float32 rounding of the model's output is all that separates it from t
    s = dict(boxes=pairs[..., [0, 1, 2, 3, 4]], sc=tm.nm.heading_sc(pairs[..., 4]), speed=pairs[..., 5], present=np.ones(pairs.shape[:2], bool))
    ttc, index = tm.time_to_collision(s['boxes'], s['sc'], s['speed'], s['present'], 1, 1, HORIZON)
    assert np.array_equal(ttc[:, 0, 0], t.astype(F32)) and np.array_equal(index[:, 0, 0], np.where(cand, 1, -1))


def ask(rows, k=1, horizon=5.0, margin=0.0, A=1):
    s = tm.scene([rows])
    ttc, index = tm.time_to_collision(s['boxes'], s['sc'], s['speed'], s['present'], A, k, horizon, margin)
    return ttc[0].tolist(), index[0].tolist()


def test_head_on_rear_end_and_crossing():
    # (x, y, length, width, quarter turns, speed, present)
    assert ask([(0, 0, 4, 2, 0, 10, 1), (50, 0, 4, 2, 2, 10, 1)]) == ([[float(F32(2.3))]], [[1]])                 # 46 m gap closing at 20 m/s
    assert ask([(0, 0, 4, 2, 0, 10, 1), (50, 0, 4, 2, 2, 10, 1)], horizon=2.0) == ([[INF]], [[-1]])
    assert ask([(0, 0, 4, 2, 0, 10, 1), (10, 0, 4, 2, 0, 10, 1)], horizon=INF) == ([[INF]], [[-1]])               # equal speeds: never
    assert ask([(0, 0, 4, 2, 0, 10, 1), (10, 0, 4, 2, 0, 8, 1)], horizon=INF) == ([[3.0]], [[1]])                 # 6 m gap closing at 2 m/s
    assert ask([(0, 0, 4, 2, 0, 8, 1), (10, 0, 4, 2, 0, 10, 1)], horizon=INF) == ([[INF]], [[-1]])                # the leader is faster
    # a crossing at right angles: the other comes from the south and its front reaches the observer's side when the observer is there
    assert ask([(0, 0, 4, 2, 0, 10, 1), (20, -20, 4, 2, 1, 10, 1)]) == ([[float(F32(1.7))]], [[1]])               # both need 1.7 s
    assert ask([(0, 0, 4, 2, 0, 10, 1), (20, -20, 4, 2, 1, 2, 1)]) == ([[INF]], [[-1]])                           # the observer is through first
    # both ways round give the same time
    assert ask([(50, 0, 4, 2, 2, 10, 1), (0, 0, 4, 2, 0, 10, 1)]) == ([[float(F32(2.3))]], [[1]])


def test_parallel_lanes_and_the_margin():
    lanes = [(0, 0, 4.5, 1.5, 0, 12, 1), (30, 3.5, 4.5, 1.5, 2, 9, 1)]                                           # 3.5 m apart, 1.5 m wide: 2 m clear
    assert ask(lanes, horizon=INF) == ([[INF]], [[-1]])
    assert ask(lanes, horizon=INF, margin=1.0) == ([[INF]], [[-1]])                                              # 1 m clear still
    wide = [(0, 0, 4.5, 2, 0, 12, 1), (1, 3.5, 4.5, 2, 2, 9, 1)]                                                 # 2 m wide, alongside: 1.5 m clear
    assert ask(wide, horizon=INF) == ([[INF]], [[-1]])
    assert ask(wide, margin=0.8)[1] == [[-1]]                                                                    # 0.7 m clear
    assert ask([(0, 0, 4.5, 2, 0, 12, 1), (1, 2.75, 4.5, 2, 2, 9, 1)], margin=0.8) == ([[0.0]], [[1]])            # 0.75 m clear: it touches at once
    # the margin grows the observer alone: the same pair the other way round asks for the other's margin
    assert ask([(0, 0, 4, 2, 0, 10, 1), (10, 0, 4, 2, 0, 8, 1)], horizon=INF, margin=1.0) == ([[2.5]], [[1]])      # 5 m gap closing at 2 m/s
    assert ask([(0, 0, 4, 2, 0, 10, 1), (10, 0, 4, 2, 0, 8, 1)], horizon=INF, margin=-1.0) == ([[3.5]], [[1]])     # the arithmetic decides


def test_overlapping_pairs_are_at_zero_and_never_negative_zero():
    ttc, index = ask([(0, 0, 4, 2, 0, 5, 1), (3, 1, 4, 2, 1, 5, 1), (1, 0, 4, 2, 0, 30, 1)], k=2)
    assert index == [[1, 2]] and ttc == [[0.0, 0.0]]
    assert np.array(ttc, F32).view(np.uint32).tolist() == [[0, 0]]                                               # +0.0: lo was -0.0 for entity 1
    assert ask([(0, 0, 4, 2, 0, 0, 1), (0, 0, 4, 2, 0, 0, 1)]) == ([[0.0]], [[1]])                                # coincident and standing


def test_a_contact_exactly_at_the_horizon_and_a_float64_step_beyond():
    a = [0.0, 0.0, 4.0, 2.0, 0.0, 1.0, 1.0]                                                                      # (x, y, l, w, s, c, v): east at 1 m/s
    far = np.nextafter(7.0, 8.0)
    e = [np.array([7.0, far]), np.zeros(2), np.full(2, 4.0), np.full(2, 2.0), np.zeros(2), np.ones(2), np.zeros(2)]
    possible, lo, hi = tm.pair_interval(a, e)
    assert lo[0] == 3.0 and lo[1] > 3.0 and lo[1] - 3.0 <= 2 * np.spacing(3.0)
    cand, ttc = tm.pair_ttc(a, e, 3.0)
    assert cand.tolist() == [True, False] and ttc.tolist() == [3.0, INF]
    assert tm.pair_ttc(a, e, np.nextafter(F32(3.0), F32(4.0)))[0].tolist() == [True, True]
    assert tm.pair_ttc(a, e, 0.0)[0].tolist() == [False, False] and tm.pair_ttc(a, e, INF)[0].tolist() == [True, True]


def test_nan_absent_slots_and_ties():
    rows = [(0, 0, 4, 2, 0, 10, 1), (50, 0, 4, 2, 2, 10, 1), (26, -26, 4, 2, 1, 10, 1), (np.nan, 0, 4, 2, 0, 0, 1), (20, 0, 4, 2, 0, 0, 0)]
    ttc, index = ask(rows, k=4)
    t = float(F32(2.3))
    assert index == [[1, 2, -1, -1]] and ttc == [[t, t, INF, INF]]                    # the tie by the lower index; the NaN and the absent one are nobody
    assert ask(rows, k=1) == ([[t]], [[1]])
    assert ask(rows[::-1], k=2, A=2) == ([[INF, INF], [INF, INF]], [[-1, -1], [-1, -1]])                          # an absent and a NaN observer
    for col in range(6):                                                                                         # any of the values
        for bad in (np.nan, np.inf, -np.inf):
            r = [list(q) for q in rows[:2]]
            r[1][col] = bad
            if col == 4:                                                                                         # (the heading reaches the kernel as sin, cos)
                s = tm.scene([rows[:2]])
                s['sc'][0, 1, 0] = bad
                assert tm.time_to_collision(s['boxes'], s['sc'], s['speed'], s['present'], 1, 1, 5.0)[1].tolist() == [[[-1]]]
            else:
                assert ask(r)[1] == [[-1]], (col, bad)
    assert ask([rows[0], rows[1]], k=32)[1][0] == [1] + [-1] * 31


def test_the_definition_cases():
    c = tm.definition_cases()
    ttc, index = tm.time_to_collision(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, tm.DEFINITION_HORIZON)
    assert index.tolist() == tm.DEFINITION_INDEX
    assert np.array_equal(ttc, np.array(tm.DEFINITION_TTC, F32))
    assert ttc[0, 1, 0] < ttc[0, 1, 1] == F32(1.2)                                     # a float32 step apart at the input, two distinct times
    visible = np.ones((2, 3, 6), bool)
    visible[0, 0, 1] = False
    assert tm.time_to_collision(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, 3.0, visible=visible)[1][0, 0].tolist() == [3, 4, -1, -1]


@pytest.mark.parametrize('name', sorted(tm.SCENES))
def test_the_random_scenes_of_the_device_tests_are_not_empty(name):
    """at least a quarter of the present observers has a finite time, at least one time is 0 and at least one above 0: the bit comparison on the
    device cannot pass on empty rows"""
    s, A = tm.scenes(name)
    ttc, index = tm.time_to_collision(s['boxes'], s['sc'], s['speed'], s['present'], A, 32, tm.COVERAGE_HORIZON)
    present = s['present'][:, :A]
    finite = np.isfinite(ttc[..., 0])
    assert not finite[~present].any() and np.isnan(s['speed'][:, -1]).all()
    assert 4 * finite.sum() >= present.sum() > 0 and (ttc == 0).any() and ((ttc > 0) & np.isfinite(ttc)).any(), (name, int(finite.sum()), int(present.sum()))
