"""The registers, LDS and scratch the time-to-collision kernel ends at, asserted on the BUILT product: tools/kernel_resources.py
reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from test_neighbors_resources import frame  # noqa: E402


@pytest.fixture(scope='module')
def kernel():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert 'time_to_collision_kernel' in table, 'libtdship.so holds no time_to_collision_kernel'
    return table['time_to_collision_kernel']


def test_the_kernel_needs_no_stack(kernel):
    """nothing in it needs scratch: no spills, no private arrays (the keys of a large scene live in LDS, not in a per-thread array)"""
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel


def test_the_kernel_keeps_its_occupancy(kernel):
    """the bounds DESIGN.md 5.5k states: 80 VGPRs in this build (the pair test is binary64: two registers a value), held at <= 96 -- five waves
    per SIMD, the next step of the occupancy table, as the neighbour kernel's 36 are held at 64 --, at most 104 SGPRs, wave64, workgroups of
    256, no static LDS"""
    assert kernel['vgpr_count'] <= 96 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] >= 5, kernel
    assert kernel['sgpr_count'] <= 104, kernel
    assert kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64 and kernel['group_segment_fixed_size'] == 0, kernel


def test_the_dynamic_lds_of_a_launch_is_what_the_design_states():
    """32 bytes per entity, and above 64 entities a row of 4-byte keys per wave: 2 KiB for the workload's 64 entities, 48 KiB at the limit of
    TDS_TTC_MAX_ENTITIES -- within the 64 KiB a launch gets without asking for more.  Read from the constants the launch is sized by
    (csrc/tds_observers.h), with the key rows."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'ttc.hip')).read()
    lds = frame()
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    limit = int(re.search(r'#define TDS_TTC_MAX_ENTITIES (\d+)', header).group(1))
    assert limit == 1024 and 'tds::slice_grid(B, A), dim3(tds::OBS_BLOCK), tds::lds_bytes(E, true)' in src and 'TDS_TTC_MAX_ENTITIES' in src
    assert lds(64, True) == 2 * 1024 and lds(65, True) == 65 * 48 and lds(limit, True) == 48 * 1024 <= 64 * 1024
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('### 5.5k'):]
    assert '32 bytes' in section and '48 KiB' in section and '2 KiB' in section
