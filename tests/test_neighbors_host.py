"""CPU-only checks of the neighbour observations' host side: bad arguments and CPU tensors are refused before anything is launched, the library
reports its size rules through the C ABI without a launch, and `Neighbors.mask` / `Neighbors.take` on hand-made tensors."""
import os
import re

import pytest
import torch

from test_host_logic import make_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_inputs(B=2, A=3, E=5):
    return torch.zeros(B, E, 5), torch.zeros(B, E, 2), torch.zeros(B, E), torch.ones(B, E, dtype=torch.bool)


@pytest.mark.parametrize('kwargs', [dict(k=0), dict(k=33), dict(k=-1), dict(k=2.5), dict(max_distance=-1.0), dict(max_distance=float('nan'))])
def test_bad_arguments_raise_before_any_launch(kwargs):
    """a ValueError about the argument, on a CPU simulator and on CPU tensors: raised before the device is even looked at"""
    from torchdrivesim_amd import _ops
    with pytest.raises(ValueError, match='neighbors'):
        make_sim().compute_neighbors(**kwargs)
    with pytest.raises(ValueError, match='neighbors'):
        _ops.neighbors(*cpu_inputs(), 3, kwargs.get('k', 8), kwargs.get('max_distance', 50.0))
    with pytest.raises(ValueError, match='neighbors'):
        _ops.check_neighbors_args(kwargs.get('k', 8), kwargs.get('max_distance', 50.0))


def test_the_limits_of_k_and_an_infinite_radius_pass_the_host_rules():
    from torchdrivesim_amd import _native, _ops
    assert _native.NEIGHBORS_MAX_K == 32 and _native.NEIGHBORS_MAX_ENTITIES == 1024
    for k, d in ((1, 0.0), (32, 50.0), (8, float('inf'))):
        _ops.check_neighbors_args(k, d)
    src = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    assert int(re.search(r'#define TDS_NEIGHBORS_MAX_K (\d+)', src).group(1)) == _native.NEIGHBORS_MAX_K
    assert int(re.search(r'#define TDS_NEIGHBORS_MAX_ENTITIES (\d+)', src).group(1)) == _native.NEIGHBORS_MAX_ENTITIES


def test_wrong_shapes_are_refused():
    from torchdrivesim_amd import _ops
    boxes, sc, speed, present = cpu_inputs()
    for visible in (torch.ones(2, 3, 4, dtype=torch.bool), torch.ones(2, 5, 5, dtype=torch.bool), torch.ones(3, 5, dtype=torch.uint8)):
        with pytest.raises(ValueError, match='visible must be'):
            _ops.neighbors(boxes, sc, speed, present, 3, 8, 50.0, visible=visible)
    with pytest.raises(ValueError, match='visible must be bool or uint8'):
        _ops.neighbors(boxes, sc, speed, present, 3, 8, 50.0, visible=torch.ones(2, 3, 5))
    with pytest.raises(ValueError, match='exposed agents'):
        _ops.neighbors(boxes, sc, speed, present, 6, 8, 50.0)
    with pytest.raises(ValueError, match='speed and present'):
        _ops.neighbors(boxes, sc, speed[:, :4], present, 3, 8, 50.0)
    with pytest.raises(ValueError, match='boxes must be'):
        _ops.neighbors(boxes[..., :4], sc, speed, present, 3, 8, 50.0)


def test_cpu_tensors_raise():
    from torchdrivesim_amd import _ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim(2, 3, npc=2).compute_neighbors()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim().compute_neighbors(k=1, max_distance=float('inf'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.neighbors(*cpu_inputs(), 3, 8, 50.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.neighbors(*cpu_inputs(), 3, 8, 50.0, visible=torch.ones(2, 3, 5, dtype=torch.bool))


def test_the_library_reports_bad_arguments_loudly_without_a_launch():
    """through the C ABI with null pointers and no GPU: TDS_EINVAL or TDS_ELIMIT and a message that names the rule"""
    from torchdrivesim_amd import _native
    L = _native.lib()
    call = lambda B=1, A=1, E=2, K=8, d=50.0: L.tds_neighbors_f32(None, None, None, None, None, None, None, B, A, E, K, d, None)
    for kw, word in ((dict(K=0), 'K must be'), (dict(K=33), 'K must be'), (dict(d=-1.0), 'max_distance'), (dict(d=float('nan')), 'max_distance'),
                     (dict(A=3, E=2), 'exposed'), (dict(B=-1), 'bad sizes')):
        assert call(**kw) == _native.E_INVAL and word in _native.last_error(), (kw, _native.last_error())
    assert call(E=1025) == _native.E_LIMIT and 'LDS' in _native.last_error()
    assert call(B=0) == 0 and call(A=0) == 0 and call(A=0, E=0) == 0           # nothing to do is not an error
    assert call(d=float('inf')) == _native.E_INVAL and 'null pointer' in _native.last_error()      # the radius passed; the pointers did not


def test_mask_and_take_on_hand_made_tensors():
    from torchdrivesim_amd.simulator import Neighbors
    assert Neighbors.FEATURES == ('x', 'y', 'sin', 'cos', 'vx', 'vy', 'length', 'width')
    index = torch.tensor([[[2, 0, -1], [1, -1, -1]], [[3, 2, 1], [-1, -1, -1]]], dtype=torch.int32)      # B = 2, A = 2, K = 3 of E = 4
    nb = Neighbors(torch.zeros(2, 2, 3, 8), index)
    assert nb.mask.tolist() == [[[True, True, False], [True, False, False]], [[True, True, True], [False, False, False]]]
    kind = torch.tensor([[10, 11, 12, 13], [20, 21, 22, 23]])
    assert nb.take(kind).tolist() == [[[12, 10, 0], [11, 0, 0]], [[23, 22, 21], [0, 0, 0]]]
    assert nb.take(kind, fill=-7).tolist() == [[[12, 10, -7], [11, -7, -7]], [[23, 22, 21], [-7, -7, -7]]]
    state = torch.arange(2 * 4 * 3, dtype=torch.float32).reshape(2, 4, 3)
    got = nb.take(state, fill=float('nan'))
    assert got.shape == (2, 2, 3, 3) and torch.equal(got[0, 0, 0], state[0, 2]) and torch.equal(got[1, 0, 2], state[1, 1])
    assert bool(got[0, 0, 2].isnan().all()) and bool(got[1, 1].isnan().all()) and got.dtype == state.dtype
    assert nb.take(kind.bool()).dtype == torch.bool
    with pytest.raises(ValueError, match='take'):
        nb.take(torch.zeros(3, 4))


def test_the_kernel_source_neither_allocates_nor_synchronises():
    csrc = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
    for name in ('neighbors.hip', 'tds_observers.h'):                        # the kernel and the frame it launches in
        src = re.sub(r'//.*', '', open(os.path.join(csrc, name)).read())
        for word in ('hipMalloc', 'hipFree', 'hipMemset', 'hipMemcpy', 'Synchronize', 'hipHostMalloc', 'asm', 'atomic'):
            assert word not in src, f'{name} mentions {word}'
    assert open(os.path.join(csrc, 'neighbors.hip')).read().count('hipLaunchKernelGGL') == 1                             # one launch,
    assert 'hipLaunchKernelGGL' not in open(os.path.join(csrc, 'tds_observers.h')).read()                                # and none in the frame
    make = open(os.path.join(csrc, 'Makefile')).read()
    assert '-ffp-contract=off' in make and 'neighbors.hip' in make and make.count('tds_observers.h') == 2
