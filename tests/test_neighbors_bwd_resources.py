"""The registers, LDS and scratch the backward kernel of the neighbour observations ends at, asserted on the BUILT product:
tools/kernel_resources.py reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc
cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from test_neighbors_resources import frame  # noqa: E402
KERNEL = 'neighbors_bwd_kernel'


@pytest.fixture(scope='module')
def kernel():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert KERNEL in table, 'libtdship.so holds no backward kernel of the neighbour observations'
    return table[KERNEL]


def test_the_kernel_needs_no_stack(kernel):
    """nothing in it needs scratch: no spills, no private arrays (the 14 contributions and the seven sums are indexed by constants alone)"""
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel


def test_the_kernel_keeps_its_occupancy(kernel):
    """the bounds DESIGN.md 5.5n states: 60 VGPRs in this build, held at <= 64 -- eight waves per SIMD, the step of the occupancy table just
    above and the most there are; 46 SGPRs, held below the 104 at which they would start to cost waves; wave64, workgroups of 256, no static LDS"""
    assert kernel['vgpr_count'] <= 64 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] >= 8, kernel
    assert kernel['sgpr_count'] <= 104, kernel
    assert kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64 and kernel['group_segment_fixed_size'] == 0, kernel


def test_the_dynamic_lds_of_a_launch_is_what_the_design_states():
    """32 bytes per entity and nothing else: 2 KiB for the workload's 64 entities, 32 KiB at the limit of TDS_NEIGHBORS_MAX_ENTITIES -- within
    the 64 KiB a launch gets without asking for more.  Read from the constants the launch is sized by (csrc/tds_observers.h), without key rows."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'neighbors_bwd.hip')).read()
    lds = frame()
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    limit = int(re.search(r'#define TDS_NEIGHBORS_MAX_ENTITIES (\d+)', header).group(1))
    assert limit == 1024 and 'tds::slice_grid(B, E), dim3(tds::OBS_BLOCK), tds::lds_bytes(E, false)' in src and 'TDS_NEIGHBORS_MAX_ENTITIES' in src
    assert all(lds(E, False) == E * 32 for E in (1, 64, 65, limit)) and lds(64, False) == 2 * 1024 and lds(limit, False) == 32 * 1024 <= 64 * 1024
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('### 5.5n'):]
    assert '32 bytes' in section and '32 KiB' in section and '2 KiB' in section and '60 VGPRs' in section and '46 SGPRs' in section
