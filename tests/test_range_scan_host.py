"""CPU-only checks of the range scan's host side: the two entry points in the header and the binding, the ray angles, and that bad arguments
and CPU tensors are refused before anything is launched."""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_host_logic import make_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_arguments(name):
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tdship.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
    assert m, f'{name} is not declared in include/tdship.h'
    return [a.strip() for a in m.group(1).split(',')]


def test_header_declares_both_entry_points_and_the_binding_matches():
    import ctypes
    from torchdrivesim_amd import _native
    single, multi = declared_arguments('tds_range_scan_f32'), declared_arguments('tds_range_scan_multi_f32')
    assert len(single) == 15 and len(multi) == 16
    assert multi[2:] == single[1:] and 'tds_mapset_t' in multi[0] and 'scene_map' in multi[1] and 'tds_map_t' in single[0]
    for name, args in (('tds_range_scan_f32', single), ('tds_range_scan_multi_f32', multi)):
        sig = _native._SIGNATURES[name]
        assert len(sig) == len(args)
        for ctype, arg in zip(sig, args):
            want = ctypes.c_void_p if '*' in arg else {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float': ctypes.c_float}[arg.split()[0]]
            assert ctype is want, (name, arg, ctype)
        assert hasattr(_native.lib(), name)
    assert _native.lib().tds_range_scan_f32.restype is ctypes.c_int
    assert re.search(r'#define TDS_SCAN_MAX_ENTITIES (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read())


def test_range_scan_angles_match_the_formula():
    from torchdrivesim_amd.simulator import Simulator
    for R, fov in ((1, 2 * math.pi), (16, 2 * math.pi), (64, math.pi / 2), (100, 1.0)):
        got = Simulator.range_scan_angles(R, fov)
        want = np.array([-fov / 2 + fov * (k + 0.5) / R for k in range(R)])
        assert got.dtype == torch.float32 and tuple(got.shape) == (R,)
        assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert Simulator.range_scan_angles(1)[0] == 0.0                        # one ray looks straight ahead
    a = Simulator.range_scan_angles(64).numpy()
    assert np.all(np.diff(a) > 0) and abs(a[0] + a[-1]) < 1e-6 and a[0] > -math.pi and a[-1] < math.pi   # counter-clockwise, symmetric
    assert make_sim().range_scan_angles(8).shape == (8,)


@pytest.mark.parametrize('kwargs', [dict(n_rays=0), dict(n_rays=-3), dict(n_rays=2.5), dict(max_range=-1.0), dict(max_range=float('inf')),
                                    dict(max_range=float('nan')), dict(gap_tolerance=-0.01), dict(gap_tolerance=float('nan')), dict(fov=0.0),
                                    dict(fov=float('nan')), dict(max_range=1e39)])
def test_bad_arguments_raise_before_any_launch(kwargs):
    """a ValueError about the argument, on a CPU simulator: raised before the device is even looked at"""
    with pytest.raises(ValueError, match='range scan'):
        make_sim().compute_range_scan(**kwargs)


def test_compute_range_scan_on_cpu_tensors_raises():
    from torchdrivesim_amd import _ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim(2, 3, npc=2).compute_range_scan()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim().compute_range_scan(n_rays=8, road=False, agents=False)
    B, A, E, R = 2, 3, 5, 4
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.range_scan(None, torch.zeros(B, E, 5), torch.zeros(B, E, 2), torch.ones(B, E, dtype=torch.bool), torch.zeros(B, A, R, 2), A, 50.0, 0.02)
    # shapes that do not fit are refused too
    with pytest.raises(ValueError, match='exposed agents'):
        _ops.range_scan(None, torch.zeros(B, 2, 5), torch.zeros(B, 2, 2), torch.ones(B, 2, dtype=torch.bool), torch.zeros(B, A, R, 2), A, 50.0, 0.02)


def test_the_library_reports_bad_sizes_loudly_without_a_launch():
    """through the C ABI with null pointers and no GPU: every size rule fails with TDS_EINVAL (or TDS_ELIMIT) and a message that names it"""
    from torchdrivesim_amd import _native
    L = _native.lib()
    call = lambda B=1, A=1, E=1, R=8, max_range=50.0, gap=0.02: L.tds_range_scan_f32(None, None, None, None, None, None, None, None, B, A, E, R, max_range, gap, None)
    for kw, word in ((dict(R=0), 'rays'), (dict(R=-1), 'rays'), (dict(A=3, E=2), 'exposed'), (dict(max_range=-1.0), 'max_range'),
                     (dict(max_range=float('inf')), 'max_range'), (dict(max_range=float('nan')), 'max_range'), (dict(gap=-1.0), 'gap_tolerance'),
                     (dict(gap=float('nan')), 'gap_tolerance'), (dict(B=-1), 'bad sizes')):
        assert call(**kw) == _native.E_INVAL and word in _native.last_error(), (kw, _native.last_error())
    assert call(E=100000, A=1) == _native.E_LIMIT and 'LDS' in _native.last_error()
    assert call(B=0) == 0 and call(A=0) == 0                               # nothing to do is not an error
    assert L.tds_range_scan_multi_f32(None, None, None, None, None, None, None, None, None, 1, 1, 1, 8, 50.0, 0.02, None) == _native.E_INVAL
    assert 'map set' in _native.last_error()
    with pytest.raises(_native.TdsError, match='tds_range_scan_f32'):
        _native.check(call(R=0), 'tds_range_scan_f32')


def test_the_scan_kernel_source_neither_allocates_nor_synchronises():
    src = re.sub(r'//.*', '', open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'scan.hip')).read())
    for word in ('hipMalloc', 'hipFree', 'hipMemset', 'hipMemcpy', 'Synchronize', 'hipHostMalloc'):
        assert word not in src, f'scan.hip mentions {word}'
    assert '-ffp-contract=off' in open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'Makefile')).read()
    assert 'scan.hip' in open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'Makefile')).read()
