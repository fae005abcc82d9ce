"""CPU-only checks of the host side of the differentiable lane observations: the library reports the argument rules of its backward entry point
through the C ABI without a launch, bad arguments and CPU tensors are refused by the Python wrapper and by the Simulator before anything is
launched, the header text and the derived signature agree, and the sources keep their promises (one launch, nothing allocated, no atomics,
nothing of HIP in the header of the formulas, the shared device code stated once)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from test_host_logic import make_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
INF, NAN = float('inf'), float('nan')
NAME = 'tds_lane_observations_bwd_multi'


class LaneSet(ctypes.Structure):
    """`tds_laneset` of csrc/tds_lanes.h, which the entry point reads n and max_lanelets of before it launches anything: a stand-in made on the
    host, so that the rules behind the null check can be reached without a GPU (nothing here is ever launched on)"""
    _fields_ = [('d_views', ctypes.c_void_p), ('n', ctypes.c_int), ('device', ctypes.c_int), ('max_tol', ctypes.c_float), ('max_lanelets', ctypes.c_int)]


def test_the_stand_in_has_the_fields_of_the_library():
    src = open(os.path.join(CSRC, 'tds_lanes.h')).read()
    body = re.search(r'struct tds_laneset \{(.*?)\};', src, flags=re.S).group(1)
    body = re.sub(r'//.*', '', body)
    assert re.sub(r'\s+', ' ', body).strip() == 'tds::LaneView *d_views; int n, device; float max_tol; int max_lanelets;'


def test_the_library_reports_bad_arguments_loudly_without_a_launch():
    """through the C ABI with null pointers and no GPU: TDS_EINVAL or TDS_ELIMIT and a message that names the rule -- K8's rules"""
    from torchdrivesim_amd import _native
    L = _native.lib()
    fn = getattr(L, NAME)

    def call(B=1, A=1, K=1, P=1, spacing=4.0, tables=1, lanelets=10, scene_map=None, null_set=False):
        s = LaneSet(None, tables, 0, 1.0, lanelets)
        return fn(None if null_set else ctypes.addressof(s), scene_map, None, None, None, None, None, None, None, B, A, K, P, spacing, None)

    for kw, word in ((dict(null_set=True), 'set is null'), (dict(K=0), 'K must be'), (dict(K=33), 'K must be'), (dict(K=-1), 'K must be'),
                     (dict(P=0), 'P must be'), (dict(P=33), 'P must be'), (dict(spacing=0.0), 'spacing'), (dict(spacing=-1.0), 'spacing'),
                     (dict(spacing=INF), 'spacing'), (dict(spacing=NAN), 'spacing'), (dict(B=-1), 'bad sizes'), (dict(A=-1), 'bad sizes'),
                     (dict(B=1 << 31, A=2), 'bad sizes'), (dict(tables=2), 'needs scene_map')):
        assert call(**kw) == _native.E_INVAL and word in _native.last_error(), (kw, _native.last_error())
        assert NAME in _native.last_error()
    assert call(lanelets=2049) == _native.E_LIMIT and '2049 lanelets' in _native.last_error()
    assert call(lanelets=2049, K=0) == _native.E_INVAL                          # the argument rules come first
    assert call(B=0) == 0 and call(A=0) == 0 and call(B=0, A=0, K=32, P=32) == 0     # B * A == 0: nothing to do is not an error
    for kw in (dict(), dict(K=32, P=32, lanelets=2048)):                         # these pass the rules; the pointers do not
        assert call(**kw) == _native.E_INVAL and 'null pointer' in _native.last_error(), kw


def test_the_entry_point_is_declared_once_and_as_the_header_states_it():
    from torchdrivesim_amd import _native
    assert [k for k, _ in _native.DECLARATIONS[NAME]] == ['handle', 'i32*', 'f32*', 'f32*', 'i32*', 'f32*', 'f32*', 'f32*', 'f32*', 'int64', 'int64', 'int',
                                                         'int', 'float', 'stream']
    assert [p for _, p in _native.DECLARATIONS[NAME]] == ['set', 'scene_map', 'agent_xy', 'agent_sc', 'index', 'g_features', 'g_points', 'g_xy', 'g_sc', 'B', 'A',
                                                         'K', 'P', 'spacing', 'stream']
    assert open(os.path.join(ROOT, 'torchdrivesim_amd', '_native.py')).read().count(NAME + '(') == 1
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    flat = re.sub(r'\s+', ' ', header)
    assert ('int tds_lane_observations_bwd_multi(const tds_laneset_t *set, const int32_t *scene_map, const float *agent_xy, const float *agent_sc, '
            'const int32_t *index, const float *g_features, const float *g_points, float *g_xy, float *g_sc, int64_t B, int64_t A, int K, int P, '
            'float spacing, void *stream);') in flat
    assert header.count(NAME + '(') == 1 and '* K8b ' in header
    assert '"K8b"' in open(os.path.join(CSRC, 'tds_lane_obs_grad.h')).read() and '"K8b"' in open(os.path.join(CSRC, 'lane_obs_bwd.hip')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '### 5.5o' in design and NAME in design[design.index('### 5.5o'):]


@pytest.mark.parametrize('kwargs', [dict(k=0), dict(k=33), dict(k=2.5), dict(n_points=0), dict(n_points=33), dict(spacing=0.0), dict(spacing=NAN),
                                    dict(max_distance=-1.0), dict(max_distance=NAN)])
def test_bad_arguments_raise_before_any_launch(kwargs):
    from torchdrivesim_amd import _ops
    with pytest.raises(ValueError, match='lanes: '):
        make_sim().compute_lanes(differentiable=True, **kwargs)
    kw = dict(dict(k=1, n_points=1, spacing=4.0, max_distance=30.0), **kwargs)
    xy = torch.zeros(2, 3, 2, requires_grad=True)
    with pytest.raises(ValueError, match='lanes: '):
        _ops.lane_observations_grad(None, xy, torch.zeros(2, 3, 2), torch.ones(2, 3, dtype=torch.bool), kw['k'], kw['n_points'], kw['spacing'], kw['max_distance'])


def test_wrong_shapes_and_cpu_tensors_are_refused():
    from torchdrivesim_amd import _ops
    xy, sc, present = torch.zeros(2, 3, 2, requires_grad=True), torch.zeros(2, 3, 2), torch.ones(2, 3, dtype=torch.bool)
    with pytest.raises(ValueError, match='lanes: agent_xy must be'):
        _ops.lane_observations_grad(None, xy[..., :1], sc, present, 1, 1, 4.0, 30.0)
    with pytest.raises(ValueError, match='lanes: agent_sc must be'):
        _ops.lane_observations_grad(None, xy, sc[:, :2], present, 1, 1, 4.0, 30.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.lane_observations_grad(None, xy, sc, present, 1, 1, 4.0, 30.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        make_sim(2, 3).compute_lanes(differentiable=True)


def test_the_flag_is_off_by_default_and_the_docstring_states_the_rules():
    from torchdrivesim_amd.simulator import Lanes, Simulator
    sig = inspect.signature(Simulator.compute_lanes)
    assert sig.parameters['differentiable'].default is False and list(sig.parameters)[-1] == 'differentiable'
    doc = Simulator.compute_lanes.__doc__
    assert 'No gradient' not in doc and 'contribute exactly zero' in doc and 'Constants of differentiation' in doc and 'slides' in doc
    assert 'differentiable=True' in Lanes.__doc__ and 'n_valid' in Lanes.__doc__.split('differentiable=True')[1]


def test_the_kernel_source_neither_allocates_nor_synchronises():
    for name in ('lane_obs_bwd.hip', 'tds_lane_obs_grad.h', 'tds_lane_obs.h'):
        src = re.sub(r'//.*', '', open(os.path.join(CSRC, name)).read())
        for word in ('hipMalloc', 'hipFree', 'hipMemset', 'hipMemcpy', 'Synchronize', 'hipHostMalloc', 'asm', 'atomic', '__syncthreads', '__shared__'):
            assert word not in src, f'{name} mentions {word}'
    assert open(os.path.join(CSRC, 'lane_obs_bwd.hip')).read().count('hipLaunchKernelGGL') == 1                              # one launch
    make = open(os.path.join(CSRC, 'Makefile')).read()
    assert '-ffp-contract=off' in make and ' lane_obs_bwd.hip' in make and make.count('tds_lane_obs_grad.h') == 2 and make.count('tds_lane_obs.h') == 2


def test_the_shared_device_code_exists_once():
    """the foot by a whole wave, the candidate rule and the walk with its point: in tds_lane_obs.h, which both kernels include, and nowhere else"""
    shared = open(os.path.join(CSRC, 'tds_lane_obs.h')).read()
    forward, backward = open(os.path.join(CSRC, 'lane_obs.hip')).read(), open(os.path.join(CSRC, 'lane_obs_bwd.hip')).read()
    for definition in ('bool usable(const LaneView &v, int l, const LaneRec &r)', 'bool wave_foot(', 'bool lane_point('):
        assert shared.count(definition) == 1 and definition not in forward and definition not in backward
    for src in (forward, backward):
        assert '#include "tds_lane_obs.h"' in src and 'wave_foot(v, r, x, y, lane, sb, d2)' in src and 'tds::lane_point(v, cur,' in src
        assert 'succ_items' not in src and 'segment_of' not in src
