"""CPU-only checks of the host side of the differentiable range scans: the library reports the argument rules of its backward entry points through
the C ABI without a launch, bad arguments and CPU tensors are refused by the Python wrappers and by the Simulator before anything is launched,
and the sources keep their promises (one launch, nothing allocated, no atomics, nothing added to memory)."""
import inspect
import os
import re

import pytest
import torch

from test_host_logic import make_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float('inf'), float('nan')
NAME = 'tds_range_scan_bwd_f32'


def cpu_inputs(B=2, A=3, E=5, R=4):
    return (torch.zeros(B, E, 5, requires_grad=True), torch.zeros(B, E, 2), torch.ones(B, E, dtype=torch.bool), torch.zeros(B, A, R, 2))


def test_the_library_reports_bad_arguments_loudly_without_a_launch():
    """through the C ABI with null pointers and no GPU: TDS_EINVAL or TDS_ELIMIT and a message that names the rule -- K5's rules, in K5's order"""
    import ctypes
    from torchdrivesim_amd import _native
    L = _native.lib()
    out = ctypes.c_void_p(16)                                                    # an output pointer that is never written: the rules come first

    def call(B=1, A=1, E=2, R=4, max_range=50.0, gap=0.02, g_boxes=out, multi=False):
        if multi:
            return getattr(L, 'tds_range_scan_bwd_multi_f32')(None, None, *([None] * 7), g_boxes, None, None, None, None, B, A, E, R, max_range, gap, None)
        return getattr(L, NAME)(None, *([None] * 7), g_boxes, None, None, None, None, B, A, E, R, max_range, gap, None)
    for kw, word in ((dict(R=0), 'number of rays'), (dict(R=65537), 'number of rays'), (dict(A=3, E=2), 'exposed'), (dict(B=-1), 'bad sizes'),
                     (dict(A=-1), 'bad sizes'), (dict(E=-1, A=0), 'bad sizes'), (dict(B=1 << 31), 'bad sizes'), (dict(max_range=-1.0), 'max_range'),
                     (dict(max_range=NAN), 'max_range'), (dict(max_range=INF), 'max_range'), (dict(gap=-0.5), 'gap_tolerance'), (dict(gap=NAN), 'gap_tolerance')):
        assert call(**kw) == _native.E_INVAL and word in _native.last_error(), (kw, _native.last_error())
        assert NAME in _native.last_error()
    assert call(E=1025) == _native.E_LIMIT and 'LDS' in _native.last_error()
    assert call(E=1025, R=0) == _native.E_INVAL                                  # the argument rules come first
    assert call(B=0) == 0 and call(A=0, E=0) == 0                                # B * E == 0: nothing to do is not an error
    assert call(g_boxes=None) == 0                                               # no output at all: nothing to do
    for kw in (dict(), dict(E=1024, R=65536), dict(A=0)):                        # these pass the rules; the pointers do not (A = 0 still has rows to zero)
        assert call(**kw) == _native.E_INVAL and 'null pointer' in _native.last_error(), kw
    assert call(multi=True) == _native.E_INVAL and 'tds_range_scan_bwd_multi_f32' in _native.last_error() and 'map set' in _native.last_error()


def test_the_entry_points_are_declared_once_and_as_the_header_states_them():
    from torchdrivesim_amd import _native
    tail = ['f32*', 'f32*', 'u8*', 'f32*', 'f32*', 'f32*', 'f32*', 'f32*', 'f32*', 'f32*', 'i32*', 'f32*', 'int64', 'int64', 'int64', 'int', 'float', 'float',
            'stream']
    assert [k for k, _ in _native.DECLARATIONS[NAME]] == ['handle'] + tail
    assert [k for k, _ in _native.DECLARATIONS['tds_range_scan_bwd_multi_f32']] == ['handle', 'i32*'] + tail
    source = open(os.path.join(ROOT, 'torchdrivesim_amd', '_native.py')).read()
    assert source.count(NAME + '(') == 1 and source.count('tds_range_scan_bwd_multi_f32(') == 1
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    assert 'int tds_range_scan_bwd_f32(const tds_map_t *map, const float *boxes, const float *sc, const uint8_t *present, const float *ray_sc,' in header
    assert 'int tds_range_scan_bwd_multi_f32(const tds_mapset_t *set, const int32_t *scene_map, const float *boxes,' in header
    assert '"K5b"' in open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'tds_scan_grad.h')).read() and 'K5b' in header


@pytest.mark.parametrize('kwargs', [dict(n_rays=0), dict(n_rays=65537), dict(n_rays=2.5), dict(max_range=-1.0), dict(max_range=NAN), dict(max_range=INF),
                                    dict(gap_tolerance=-1.0), dict(gap_tolerance=NAN)])
def test_bad_arguments_raise_before_any_launch(kwargs):
    from torchdrivesim_amd import _ops
    with pytest.raises(ValueError, match='range scan'):
        make_sim().compute_range_scan(differentiable=True, **kwargs)
    if 'n_rays' not in kwargs:
        for fn in (_ops.range_scan_grad, _ops.range_scan_witness):
            with pytest.raises(ValueError, match='range scan'):
                fn(None, *cpu_inputs(), 3, kwargs.get('max_range', 50.0), kwargs.get('gap_tolerance', 0.02))
    with pytest.raises(ValueError, match='fov'):
        make_sim().compute_range_scan(differentiable=True, fov=0.0)


def test_wrong_shapes_and_cpu_tensors_are_refused():
    from torchdrivesim_amd import _ops
    boxes, sc, present, ray_sc = cpu_inputs()
    for fn in (_ops.range_scan_grad, _ops.range_scan_witness):
        with pytest.raises(ValueError, match='range scan: ray_sc must be'):
            fn(None, boxes, sc, present, ray_sc[..., :1], 3, 50.0, 0.02)
        with pytest.raises(ValueError, match='range scan: 2 exposed agents'):
            fn(None, boxes, sc, present, ray_sc, 2, 50.0, 0.02)
        with pytest.raises(ValueError, match='range scan: boxes must be'):
            fn(None, boxes[..., :4], sc, present, ray_sc, 3, 50.0, 0.02)
        with pytest.raises(ValueError, match='range scan: sc must be'):
            fn(None, boxes, sc[:, :4], present, ray_sc, 3, 50.0, 0.02)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(None, boxes, sc, present, ray_sc, 3, 50.0, 0.02)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim(2, 3, npc=2).compute_range_scan(differentiable=True)


def test_the_flag_is_off_by_default_and_the_docstring_states_the_rules():
    from torchdrivesim_amd.simulator import RangeScan, Simulator
    sig = inspect.signature(Simulator.compute_range_scan)
    assert sig.parameters['differentiable'].default is False and list(sig.parameters)[-1] == 'differentiable'
    doc = Simulator.compute_range_scan.__doc__
    assert 'No gradient' not in doc and 'contributes exactly zero' in doc and 'Constants of differentiation' in doc and 'nothing is saved' in doc
    assert 'differentiable=True' in RangeScan.__doc__


def test_the_kernel_source_neither_allocates_nor_synchronises():
    csrc = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
    for name in ('scan_bwd.hip', 'tds_scan_grad.h', 'tds_scan.h'):
        src = re.sub(r'//.*', '', open(os.path.join(csrc, name)).read())
        for word in ('hipMalloc', 'hipFree', 'hipMemset', 'hipMemcpy', 'Synchronize', 'hipHostMalloc', 'atomic'):
            assert word not in src, f'{name} mentions {word}'
    src = re.sub(r'//.*', '', open(os.path.join(csrc, 'scan_bwd.hip')).read())
    assert src.count('hipLaunchKernelGGL') == 1                                  # one launch
    assert re.findall(r'asm volatile\(([^;]*)\);', src) == ['"" : "+v"(p)'], 'the one asm statement is empty: a register-class constraint, no instruction'
    make = open(os.path.join(csrc, 'Makefile')).read()
    assert '-ffp-contract=off' in make and ' scan_bwd.hip' in make and make.count('tds_scan_grad.h') == 2 and make.count('tds_scan.h') == 2
    scan = open(os.path.join(csrc, 'scan.hip')).read()
    assert '#include "tds_scan.h"' in scan and 'area2' not in scan, 'the forward takes the shared arithmetic from the header'
