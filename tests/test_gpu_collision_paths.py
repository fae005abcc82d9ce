"""
Every forward path of K2a (tds_collision_f32: the whole-scene IoU kernel and the row kernel of both metrics) against the CPU oracle and the
overlap-matrix model (tests/collision_model.py), on the shapes at which the launcher changes kernels, the 64-lane chunk loop wraps and the LDS
budget of the scene kernel ends (tests/collision_cases.py; tests/test_collision_model.py shows on the CPU that each input set contains what
it is there for).  All comparisons are exact: the kernels keep the reference's operation order per pair and its index-order sum per row, the
bit mask and the arg-max partner are integers.
"""
import numpy as np
import pytest
import torch

import collision_cases as cc
import collision_model as cm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def ops():
    from torchdrivesim_amd import _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('A,N,metric,name', cc.cases(), ids=lambda v: str(v))
def test_collision_forward_matches_oracle_and_model(ops, oracle, A, N, metric, name):
    boxes, present = cc.make(A, N, metric, name)
    bd, pd = dev(boxes), dev(present)
    sc = ops.metric_sc(torch.nan_to_num(bd, nan=0.0), metric)
    want_bits = N <= 64
    out, bits, partner = ops.collision_forward(bd, sc, pd, A, metric, want_overlap=want_bits, want_partner=True)
    plain = ops.collision_forward(bd, sc, pd, A, metric)[0]
    out, partner, plain = out.cpu().numpy(), partner.cpu().numpy(), plain.cpu().numpy()
    sc = sc.cpu().numpy()
    m = cm.model(boxes, sc, present, A, metric)
    ref = oracle.collision(boxes, present, n_exposed=A, metric=metric, sc=sc)
    np.testing.assert_array_equal(m['collision'], ref)                   # the yardsticks agree with each other on these very inputs
    cc.check_conditions(A, N, metric, name, boxes, present, m)           # ... and the set still holds what it is there for
    np.testing.assert_array_equal(out, ref)
    np.testing.assert_array_equal(partner, m['partner'])
    if want_bits:
        assert bits.dtype == torch.int64
        np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint64), m['bits'])
    np.testing.assert_array_equal(plain, out)                            # the optional outputs do not change the sum


def test_collision_forward_edges(ops):
    boxes, present = cc.make(64, 65, 'iou', 'mixed')
    bd, pd = dev(boxes), dev(present)
    sc = ops.metric_sc(bd, 'iou')
    with pytest.raises(RuntimeError):
        ops.collision_forward(bd, sc, pd, 64, 'iou', want_overlap=True)          # one bit per partner: N <= 64
    big = torch.zeros((1, 8193, 5), device=DEV)
    with pytest.raises(RuntimeError):
        ops.collision_forward(big, torch.zeros((1, 8193, 2), device=DEV), torch.ones((1, 8193), dtype=torch.bool, device=DEV), 1, 'discs')
    for metric in ('iou', 'discs'):
        out, bits, partner = ops.collision_forward(bd[:0], sc[:0], pd[:0], 64, metric, want_partner=True)
        assert out.shape == (0, 64) and partner.shape == (0, 64) and bits is None
        out, bits, partner = ops.collision_forward(bd[:, :64], sc[:, :64], pd[:, :64], 0, metric, want_overlap=True, want_partner=True)
        assert out.shape == (3, 0) and bits.shape == (3, 0) and partner.shape == (3, 0)
    torch.cuda.synchronize()
