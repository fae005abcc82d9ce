"""The registers, LDS and scratch the backward kernel of the lane observations ends at, asserted on the BUILT product:
tools/kernel_resources.py reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc
cross-compiles, no GPU involved."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
KERNEL = 'lane_obs_bwd_kernel'


@pytest.fixture(scope='module')
def kernel():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert KERNEL in table, 'libtdship.so holds no backward kernel of the lane observations'
    return table[KERNEL]


def test_the_kernel_needs_no_stack(kernel):
    """nothing in it needs scratch: no spills, no private arrays (the eight incoming gradients, the four contributions and the four sums are
    indexed by constants alone)"""
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel


def test_the_kernel_keeps_its_occupancy(kernel):
    """the bounds DESIGN.md 5.5o states: 62 VGPRs in this build, held at <= 64 -- eight waves per SIMD, the step of the occupancy table just
    above and the most there are, K8's own; 56 SGPRs, held below the 104 at which they would start to cost waves; wave64, workgroups of 256"""
    assert kernel['vgpr_count'] <= 64 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] == 8, kernel
    assert kernel['sgpr_count'] <= 104, kernel
    assert kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64, kernel


def test_the_kernel_uses_no_lds_and_the_design_states_the_figures(kernel):
    """no static LDS and none asked for at the launch: what the pairs of a slot need of its foot comes from lane k by a shuffle"""
    assert kernel['group_segment_fixed_size'] == 0, kernel
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'lane_obs_bwd.hip')).read()
    assert 'dim3(LB_BLOCK), 0, (hipStream_t)stream, g)' in src and 'constexpr int LB_BLOCK = 256;' in src and '__shared__' not in src
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('### 5.5o'):]
    assert f"{kernel['vgpr_count']} VGPRs" in section and f"{kernel['sgpr_count']} SGPRs" in section and 'no LDS' in section
    assert '62 VGPRs' in section and '56 SGPRs' in section
