"""The registers, LDS and scratch the route-goal kernels end at, asserted on the BUILT product: tools/kernel_resources.py reads the
AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
KERNELS = ('route_sample_kernel', 'route_progress_kernel', 'route_points_kernel')


@pytest.fixture(scope='module')
def kernels():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert all(k in table for k in KERNELS), 'libtdship.so holds no route-goal kernels'
    return table


def test_no_route_kernel_needs_a_stack(kernels):
    """no spills and no private arrays: a route's sixteen lanelets and offsets are read from memory where they are needed, never kept per thread"""
    for name in KERNELS:
        k = kernels[name]
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)


def test_the_progress_kernel_keeps_its_occupancy(kernels):
    """the bounds DESIGN.md 5.5d states: no LDS at all, so the registers alone set the occupancy -- at most 96 VGPRs = five waves per SIMD (it is
    built at 70), at most 104 SGPRs, workgroups of four waves = four rows"""
    k = kernels['route_progress_kernel']
    assert k['vgpr_count'] <= 96 and k['agpr_count'] == 0 and k['waves_per_simd'] >= 5, k
    assert k['sgpr_count'] <= 104, k
    assert k['max_flat_workgroup_size'] == 256 and k['wavefront_size'] == 64 and k['group_segment_fixed_size'] == 0, k


def test_the_limits_of_the_header_are_the_kernels_and_the_bindings():
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'route.hip')).read()
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    lanes = int(re.search(r'#define TDS_ROUTE_MAX_LANES (\d+)', header).group(1))
    look = int(re.search(r'#define TDS_ROUTE_MAX_LOOKAHEAD (\d+)', header).group(1))
    assert 'constexpr int ROUTE_LANES = TDS_ROUTE_MAX_LANES;' in src and 'constexpr int RBLOCK = 256;' in src
    from torchdrivesim_amd import _native
    import route_model
    assert (_native.ROUTE_MAX_LANES, _native.ROUTE_MAX_LOOKAHEAD) == (lanes, look) == (16, 32) == (route_model.MAX_LANES, route_model.MAX_LOOKAHEAD)
    assert look <= 64, 'a lookahead point per lane of one wavefront'
