"""The registers, LDS and scratch the backward kernel of the stop-line observations ends at, and what the wrong-way kernel keeps
with its one more pointer (5.5r), asserted on the BUILT product: tools/kernel_resources.py reads the AMDGPU metadata of the code objects inside
torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def table():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return kernel_resources.kernel_table(_native.LIB_PATH)


def test_the_product_holds_one_shape_of_the_kernel(table):
    """4 lanes per observer; the shapes it was measured against exist in the testing build alone"""
    assert [k for k in table if 'stop_lines_bwd_kernel' in k] == ['stop_lines_bwd_kernel<4>']


def test_the_kernel_needs_no_stack_and_no_lds(table):
    kernel = table['stop_lines_bwd_kernel<4>']
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel
    assert kernel['group_segment_fixed_size'] == 0 and 'extern __shared__' not in open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'stop_lines_bwd.hip')).read()


def test_the_kernel_keeps_its_occupancy(table):
    """60 VGPRs in this build, held at <= 64 -- eight waves per SIMD; 36 SGPRs, held below the 104 at which they would start to cost waves"""
    kernel = table['stop_lines_bwd_kernel<4>']
    assert kernel['vgpr_count'] <= 64 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] >= 8, kernel
    assert kernel['sgpr_count'] <= 104 and kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64, kernel


def test_the_wrong_way_kernel_keeps_four_waves_with_its_one_more_pointer(table):
    kernel = table['wrong_way_kernel']
    assert kernel['vgpr_count'] <= 128 and kernel['waves_per_simd'] >= 4 and kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0, kernel
