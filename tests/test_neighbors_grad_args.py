"""CPU-only checks of the host side of the differentiable neighbour observations: the library reports the argument rules of its backward entry
point through the C ABI without a launch, bad arguments and CPU tensors are refused by the Python wrapper and by the Simulator before anything is
launched, and the sources keep their promises (one launch, nothing allocated, no atomics, nothing of HIP in the header)."""
import inspect
import os
import re

import pytest
import torch

from test_host_logic import make_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float('inf'), float('nan')
NAME = 'tds_neighbors_bwd_f32'


def cpu_inputs(B=2, A=3, E=5):
    return torch.zeros(B, E, 5, requires_grad=True), torch.zeros(B, E, 2), torch.zeros(B, E), torch.ones(B, E, dtype=torch.bool)


def test_the_library_reports_bad_arguments_loudly_without_a_launch():
    """through the C ABI with null pointers and no GPU: TDS_EINVAL or TDS_ELIMIT and a message that names the rule"""
    from torchdrivesim_amd import _native
    L = _native.lib()
    call = lambda B=1, A=1, E=2, K=1: getattr(L, NAME)(None, None, None, None, None, None, None, None, B, A, E, K, None)
    for kw, word in ((dict(K=0), 'K must be'), (dict(K=33), 'K must be'), (dict(K=-1), 'K must be'), (dict(A=3, E=2), 'exposed'), (dict(B=-1), 'bad sizes'),
                     (dict(A=-1), 'bad sizes'), (dict(E=-1, A=0), 'bad sizes'), (dict(B=1 << 31), 'bad sizes')):
        assert call(**kw) == _native.E_INVAL and word in _native.last_error(), (kw, _native.last_error())
        assert NAME in _native.last_error()
    assert call(E=1025) == _native.E_LIMIT and 'LDS' in _native.last_error()
    assert call(E=1025, K=0) == _native.E_INVAL                                  # the argument rules come first
    assert call(B=0) == 0 and call(A=0, E=0) == 0                                # B * E == 0: nothing to do is not an error
    for kw in (dict(), dict(K=32, E=1024), dict(A=0)):                           # these pass the rules; the pointers do not (A = 0 still has rows to zero)
        assert call(**kw) == _native.E_INVAL and 'null pointer' in _native.last_error(), kw


def test_the_entry_point_is_declared_once_and_as_the_header_states_it():
    from torchdrivesim_amd import _native
    assert [k for k, _ in _native.DECLARATIONS[NAME]] == ['f32*', 'f32*', 'f32*', 'i32*', 'f32*', 'f32*', 'f32*', 'f32*', 'int64', 'int64', 'int64', 'int', 'stream']
    assert open(os.path.join(ROOT, 'torchdrivesim_amd', '_native.py')).read().count(NAME + '(') == 1
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    assert 'int tds_neighbors_bwd_f32(const float *boxes, const float *sc, const float *speed, const int32_t *index, const float *g_features,' in header
    assert 'float *g_boxes, float *g_sc, float *g_speed, int64_t B, int64_t A, int64_t E, int K, void *stream);' in header
    assert '"K6b"' in open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'tds_neighbors_grad.h')).read() and 'K6b' in header


@pytest.mark.parametrize('kwargs', [dict(k=0), dict(k=33), dict(k=2.5), dict(max_distance=-1.0), dict(max_distance=NAN)])
def test_bad_arguments_raise_before_any_launch(kwargs):
    from torchdrivesim_amd import _ops
    k, max_distance = kwargs.get('k', 1), kwargs.get('max_distance', 50.0)
    with pytest.raises(ValueError, match='neighbors'):
        make_sim().compute_neighbors(differentiable=True, **kwargs)
    with pytest.raises(ValueError, match='neighbors'):
        _ops.neighbors_grad(*cpu_inputs(), 3, k, max_distance)


def test_wrong_shapes_and_cpu_tensors_are_refused():
    from torchdrivesim_amd import _ops
    boxes, sc, speed, present = cpu_inputs()
    with pytest.raises(ValueError, match='neighbors: visible must be'):
        _ops.neighbors_grad(boxes, sc, speed, present, 3, 1, 50.0, torch.ones(2, 3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match='neighbors: 6 exposed agents'):
        _ops.neighbors_grad(boxes, sc, speed, present, 6, 1, 50.0)
    with pytest.raises(ValueError, match='neighbors: boxes must be'):
        _ops.neighbors_grad(boxes[..., :4], sc, speed, present, 3, 1, 50.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.neighbors_grad(boxes, sc, speed, present, 3, 1, 50.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim(2, 3, npc=2).compute_neighbors(differentiable=True)


def test_the_flag_is_off_by_default_and_the_docstring_states_the_rules():
    from torchdrivesim_amd.simulator import Neighbors, Simulator
    sig = inspect.signature(Simulator.compute_neighbors)
    assert sig.parameters['differentiable'].default is False and list(sig.parameters)[-1] == 'differentiable'
    doc = Simulator.compute_neighbors.__doc__
    assert 'No gradient' not in doc and 'contributes exactly zero' in doc and 'Constants of differentiation' in doc and 'IEEE' in doc
    assert 'differentiable=True' in Neighbors.__doc__


def test_the_kernel_source_neither_allocates_nor_synchronises():
    csrc = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
    for name in ('neighbors_bwd.hip', 'tds_neighbors_grad.h'):
        src = re.sub(r'//.*', '', open(os.path.join(csrc, name)).read())
        for word in ('hipMalloc', 'hipFree', 'hipMemset', 'hipMemcpy', 'Synchronize', 'hipHostMalloc', 'asm', 'atomic'):
            assert word not in src, f'{name} mentions {word}'
    assert open(os.path.join(csrc, 'neighbors_bwd.hip')).read().count('hipLaunchKernelGGL') == 1                         # one launch
    make = open(os.path.join(csrc, 'Makefile')).read()
    assert '-ffp-contract=off' in make and ' neighbors_bwd.hip' in make and make.count('tds_neighbors_grad.h') == 2
