"""The registers, LDS and scratch the destination-route kernels end at, asserted on the BUILT product: tools/kernel_resources.py
reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
KERNELS = ('lane_distances_kernel', 'route_to_kernel')


@pytest.fixture(scope='module')
def kernels():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert all(k in table for k in KERNELS), 'libtdship.so holds no destination-route kernels'
    return table


def test_neither_kernel_needs_a_stack(kernels):
    """no spills and no private arrays: the distance kernel's per-thread lanelets are registers (fully unrolled), a route's sixteen lanelets and
    offsets are written to memory as they are found"""
    for name in KERNELS:
        k = kernels[name]
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['max_flat_workgroup_size'] == 256 and k['wavefront_size'] == 64 and k['agpr_count'] == 0, (name, k)


def test_the_distance_field_is_the_lds(kernels):
    """one float64 per lanelet of the largest graph plus the 4-byte `changed` flag, which the field's 8-byte alignment may pad to 8: 16 KiB, so
    LDS does not limit the workgroups of a CU before the registers do"""
    from torchdrivesim_amd import _native
    lds = kernels['lane_distances_kernel']['group_segment_fixed_size']
    assert 8 * _native.ROUTE_MAX_GRAPH + 4 <= lds <= 8 * _native.ROUTE_MAX_GRAPH + 8, lds
    assert kernels['route_to_kernel']['group_segment_fixed_size'] == 0
    assert kernels['lane_distances_kernel']['vgpr_count'] <= 128, 'four waves a SIMD at least'


def test_the_limits_of_the_header_are_the_kernels_the_bindings_and_the_model():
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'route_to.hip')).read()
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    graph = int(re.search(r'#define TDS_ROUTE_MAX_GRAPH (\d+)', header).group(1))
    lanes = int(re.search(r'#define TDS_ROUTE_MAX_LANES (\d+)', header).group(1))
    assert 'constexpr int GRAPH_MAX = TDS_ROUTE_MAX_GRAPH;' in src and 'constexpr int ROUTE_LANES = TDS_ROUTE_MAX_LANES;' in src
    assert 'constexpr int DBLOCK = 256;' in src and graph % 256 == 0
    from torchdrivesim_amd import _native
    import route_to_model
    assert (_native.ROUTE_MAX_GRAPH, _native.ROUTE_MAX_LANES) == (graph, lanes) == (2048, 16) == (route_to_model.MAX_GRAPH, route_to_model.MAX_LANES)
    assert {'tds_lane_distances_f64', 'tds_route_to_multi'} <= set(_native.DECLARATIONS)
