"""
CPU checks of the K2a forward yardstick (tests/collision_model.py) and of the input sets of tests/test_gpu_collision_paths.py
(tests/collision_cases.py): the model's collision must equal the oracle's scene function bit for bit, and every set must contain what it is
there for -- judged on the model alone, so that a GPU test that passes has met ties, far partners, bit 63 and both sides of the cull.
"""
import numpy as np
import pytest

import collision_cases as cc
import collision_model as cm


def host_sc(boxes, metric):
    """[sin, cos] of the metric's angle of the scrubbed boxes, as ops.metric_sc(nan_to_num(boxes)) computes it on the device"""
    b = np.nan_to_num(boxes, nan=0.0)
    psi = b[..., 4]
    if metric == 'discs':
        psi = psi + np.float32(np.pi / 2) * (b[..., 3] > b[..., 2])
    psi = psi.astype(np.float32)
    return np.stack([np.sin(psi), np.cos(psi)], -1).astype(np.float32)


@pytest.mark.parametrize('A,N,metric,name', cc.cases(), ids=lambda v: str(v))
def test_model_equals_oracle_and_set_holds_what_it_claims(oracle, A, N, metric, name):
    boxes, present = cc.make(A, N, metric, name)
    assert boxes.shape == (cc.batch_of(N), N, 5) and boxes.dtype == np.float32
    assert N == 1 or not np.array_equal(boxes[0], boxes[1])              # the scenes of a batch differ
    sc = host_sc(boxes, metric)
    m = cm.model(boxes, sc, present, A, metric)
    np.testing.assert_array_equal(m['collision'], oracle.collision(boxes, present, n_exposed=A, metric=metric, sc=sc))
    cc.check_conditions(A, N, metric, name, boxes, present, m)


def test_dispatch_notes():
    """the `path` column of the table is derived from the launcher's own conditions"""
    assert cc.expected_path(64, 64, 'iou') == 'scene' and cc.expected_path(64, 65, 'iou') == 'row'
    assert (4 * 1024 + 6 * 682 + 2 * 6 * 682) * 4 == 65488 and cc.expected_path(6, 682, 'iou') == 'scene'
    assert (4 * 1024 + 6 * 819 + 2 * 5 * 819) * 4 == 68800 and 5 * 819 <= 4096 and cc.expected_path(5, 819, 'iou') == 'row'
    assert (4 * 1024 + 6 * 512 + 2 * 8 * 512) * 4 == 61440
    assert all(cc.expected_path(A, N, 'discs') == 'row' for (A, N), _, _ in cc.SHAPES)


def test_reductions_on_a_hand_made_matrix():
    O = np.zeros((1, 2, 66), np.float32)
    O[0, 0, [0, 5, 65]] = (1.0, 0.25, 0.25)              # self overlap; a tie across the chunk boundary -> the lowest index
    O[0, 1, [1, 65]] = (0.5, 0.75)                       # a partner larger than the self overlap, in the last chunk
    r = cm.reduce_rows(O)
    np.testing.assert_array_equal(r['partner'], [[5, 65]])
    np.testing.assert_array_equal(r['ties'], [[2, 1]])
    np.testing.assert_array_equal(r['collision'], np.float32([[0.5, 0.5]]))
    assert r['bits'] is None
    r = cm.reduce_rows(O[:, :, :64])
    np.testing.assert_array_equal(r['bits'], np.array([[1 << 5, 0]], np.uint64))
    np.testing.assert_array_equal(r['partner'], [[5, -1]])
    O = np.zeros((1, 64, 64), np.float32)
    O[0, 0, 63] = 0.5
    assert cm.reduce_rows(O)['bits'][0, 0] == np.uint64(1) << np.uint64(63)
