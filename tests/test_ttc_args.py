"""CPU-only checks of the host side of time to collision: bad arguments and CPU tensors are refused before anything is launched, the library
reports its argument rules through the C ABI without a launch, and `TimeToCollision.mask` / `.min` / `.take` on hand-made tensors."""
import os
import re

import pytest
import torch

from test_host_logic import make_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float('inf'), float('nan')


def cpu_inputs(B=2, A=3, E=5):
    return torch.zeros(B, E, 5), torch.zeros(B, E, 2), torch.zeros(B, E), torch.ones(B, E, dtype=torch.bool)


@pytest.mark.parametrize('kwargs', [dict(k=0), dict(k=33), dict(k=-1), dict(k=2.5), dict(horizon=-1.0), dict(horizon=NAN), dict(margin=NAN), dict(margin=INF),
                                    dict(margin=-INF)])
def test_bad_arguments_raise_before_any_launch(kwargs):
    """a ValueError about the argument, on a CPU simulator and on CPU tensors: raised before the device is even looked at"""
    from torchdrivesim_amd import _ops
    k, horizon, margin = kwargs.get('k', 1), kwargs.get('horizon', 5.0), kwargs.get('margin', 0.0)
    with pytest.raises(ValueError, match='time_to_collision'):
        make_sim().compute_time_to_collision(**kwargs)
    with pytest.raises(ValueError, match='time_to_collision'):
        _ops.time_to_collision(*cpu_inputs(), 3, k, horizon, margin)
    with pytest.raises(ValueError, match='time_to_collision'):
        _ops.check_ttc_args(k, horizon, margin)


def test_the_limits_pass_the_host_rules_and_the_constants_are_the_headers():
    from torchdrivesim_amd import _native, _ops
    assert _native.TTC_MAX_K == 32 and _native.TTC_MAX_ENTITIES == 1024
    for k, h, m in ((1, 0.0, 0.0), (32, 5.0, 0.5), (8, INF, -0.25)):
        _ops.check_ttc_args(k, h, m)
    src = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    assert int(re.search(r'#define TDS_TTC_MAX_K (\d+)', src).group(1)) == _native.TTC_MAX_K
    assert int(re.search(r'#define TDS_TTC_MAX_ENTITIES (\d+)', src).group(1)) == _native.TTC_MAX_ENTITIES
    assert 'int tds_time_to_collision_f32(const float *boxes, const float *sc, const float *speed, const uint8_t *present, const uint8_t *visible,' in src


def test_wrong_shapes_are_refused():
    from torchdrivesim_amd import _ops
    boxes, sc, speed, present = cpu_inputs()
    for visible in (torch.ones(2, 3, 4, dtype=torch.bool), torch.ones(2, 5, 5, dtype=torch.bool), torch.ones(3, 5, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='time_to_collision: visible must be'):
            _ops.time_to_collision(boxes, sc, speed, present, 3, 1, 5.0, visible=visible)
    with pytest.raises(ValueError, match='visible must be bool or uint8'):
        _ops.time_to_collision(boxes, sc, speed, present, 3, 1, 5.0, visible=torch.ones(2, 3, 5))
    with pytest.raises(ValueError, match='time_to_collision: 6 exposed agents'):
        _ops.time_to_collision(boxes, sc, speed, present, 6, 1, 5.0)
    with pytest.raises(ValueError, match='speed and present'):
        _ops.time_to_collision(boxes, sc, speed[:, :4], present, 3, 1, 5.0)
    with pytest.raises(ValueError, match='time_to_collision: boxes must be'):
        _ops.time_to_collision(boxes[..., :4], sc, speed, present, 3, 1, 5.0)


def test_cpu_tensors_raise():
    from torchdrivesim_amd import _ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim(2, 3, npc=2).compute_time_to_collision()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim().compute_time_to_collision(k=4, horizon=INF, margin=0.5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.time_to_collision(*cpu_inputs(), 3, 1, 5.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.time_to_collision(*cpu_inputs(), 3, 1, 5.0, 0.5, visible=torch.ones(2, 3, 5, dtype=torch.bool))


def test_the_library_reports_bad_arguments_loudly_without_a_launch():
    """through the C ABI with null pointers and no GPU: TDS_EINVAL or TDS_ELIMIT and a message that names the rule"""
    from torchdrivesim_amd import _native
    L = _native.lib()
    call = lambda B=1, A=1, E=2, K=1, h=5.0, m=0.0: L.tds_time_to_collision_f32(None, None, None, None, None, None, None, B, A, E, K, h, m, None)
    for kw, word in ((dict(K=0), 'K must be'), (dict(K=33), 'K must be'), (dict(h=-1.0), 'horizon'), (dict(h=NAN), 'horizon'), (dict(m=NAN), 'margin'),
                     (dict(m=INF), 'margin'), (dict(m=-INF), 'margin'), (dict(A=3, E=2), 'exposed'), (dict(B=-1), 'bad sizes')):
        assert call(**kw) == _native.E_INVAL and word in _native.last_error(), (kw, _native.last_error())
        assert 'tds_time_to_collision_f32' in _native.last_error()
    assert call(E=1025) == _native.E_LIMIT and 'LDS' in _native.last_error()
    assert call(E=1025, K=0) == _native.E_INVAL                                  # the argument rules come first
    assert call(B=0) == 0 and call(A=0) == 0 and call(A=0, E=0) == 0             # nothing to do is not an error
    for kw in (dict(h=INF), dict(h=0.0), dict(m=-1.0), dict(K=32, E=1024)):      # these pass the rules; the pointers do not
        assert call(**kw) == _native.E_INVAL and 'null pointer' in _native.last_error(), kw


def test_mask_min_and_take_on_hand_made_tensors():
    from torchdrivesim_amd.simulator import TimeToCollision
    index = torch.tensor([[[2, 0, -1], [1, -1, -1]], [[3, 2, 1], [-1, -1, -1]]], dtype=torch.int32)      # B = 2, A = 2, K = 3 of E = 4
    ttc = torch.tensor([[[0.0, 1.5, INF], [2.0, INF, INF]], [[0.5, 0.5, 4.0], [INF, INF, INF]]])
    t = TimeToCollision(ttc, index)
    assert t.mask.tolist() == [[[True, True, False], [True, False, False]], [[True, True, True], [False, False, False]]]
    assert t.min.tolist() == [[0.0, 2.0], [0.5, INF]] and t.min.shape == (2, 2)
    kind = torch.tensor([[10, 11, 12, 13], [20, 21, 22, 23]])
    assert t.take(kind).tolist() == [[[12, 10, 0], [11, 0, 0]], [[23, 22, 21], [0, 0, 0]]]
    assert t.take(kind, fill=-7).tolist() == [[[12, 10, -7], [11, -7, -7]], [[23, 22, 21], [-7, -7, -7]]]
    state = torch.arange(2 * 4 * 3, dtype=torch.float32).reshape(2, 4, 3)
    got = t.take(state, fill=NAN)
    assert got.shape == (2, 2, 3, 3) and torch.equal(got[0, 0, 0], state[0, 2]) and torch.equal(got[1, 0, 2], state[1, 1])
    assert bool(got[0, 0, 2].isnan().all()) and bool(got[1, 1].isnan().all()) and got.dtype == state.dtype
    with pytest.raises(ValueError, match='take'):
        t.take(torch.zeros(3, 4))


def test_the_kernel_source_neither_allocates_nor_synchronises():
    csrc = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
    for name in ('ttc.hip', 'tds_ttc.h', 'tds_observers.h'):
        src = re.sub(r'//.*', '', open(os.path.join(csrc, name)).read())
        for word in ('hipMalloc', 'hipFree', 'hipMemset', 'hipMemcpy', 'Synchronize', 'hipHostMalloc', 'asm', 'atomic'):
            assert word not in src, f'{name} mentions {word}'
    assert 'hip' not in re.sub(r'//.*', '', open(os.path.join(csrc, 'tds_ttc.h')).read()).replace('__HIPCC__', '')      # nothing of HIP in the header
    assert open(os.path.join(csrc, 'ttc.hip')).read().count('hipLaunchKernelGGL') == 1                                   # one launch,
    assert 'hipLaunchKernelGGL' not in open(os.path.join(csrc, 'tds_observers.h')).read()                                # and none in the frame
    make = open(os.path.join(csrc, 'Makefile')).read()
    assert '-ffp-contract=off' in make and ' ttc.hip' in make and 'tds_ttc.h' in make and make.count('tds_observers.h') == 2
