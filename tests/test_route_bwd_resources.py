"""The registers, LDS and scratch the route step's backward kernel ends at, asserted on the BUILT product: tools/kernel_resources.py
reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
KERNEL = 'route_progress_bwd_kernel'


@pytest.fixture(scope='module')
def kernel():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert KERNEL in table, 'libtdship.so holds no backward kernel of the route step'
    return table[KERNEL]


def test_the_backward_kernel_needs_no_stack_and_no_lds(kernel):
    """no spills, no private arrays and no LDS: the lanes exchange their partial sums by shuffles alone"""
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel
    assert kernel['group_segment_fixed_size'] == 0, kernel


def test_the_backward_kernel_keeps_the_forwards_occupancy(kernel):
    """the bounds of route_progress_kernel: at most 96 VGPRs = five waves per SIMD, at most 104 SGPRs, workgroups of four waves = four rows"""
    assert kernel['vgpr_count'] <= 96 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] >= 5, kernel
    assert kernel['sgpr_count'] <= 104, kernel
    assert kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64, kernel


def test_the_helpers_are_shared_not_copied():
    """weigh_segment and route_point are defined once, in the header both kernels include"""
    csrc = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
    read = lambda name: open(os.path.join(csrc, name)).read()
    for helper in ('bool weigh_segment(', 'void route_point('):
        assert helper in read('tds_route.h') and helper not in read('route.hip') and helper not in read('route_bwd.hip'), helper
    for name in ('route.hip', 'route_bwd.hip'):
        assert '#include "tds_route.h"' in read(name), name
    assert '__device__' not in read('tds_route_grad.h') and '__global__' not in read('tds_route_grad.h'), 'a host compiler takes the arithmetic as it is'
