"""The registers, LDS and scratch the neighbour kernel ends at, asserted on the BUILT product: tools/kernel_resources.py reads
the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def frame():
    """the constants and the LDS rule of the frame the kernel launches in, asserted on csrc/tds_observers.h -> lds(n, with_key_rows) in bytes"""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'tds_observers.h')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    assert (const['OBS_BLOCK'], const['OBS_SLICE'], const['OBS_WORDS']) == (256, 16, 8) and 'OBS_WAVES = OBS_BLOCK / 64' in src
    assert 'return (size_t)n * OBS_WORDS * sizeof(float) + (with_key_rows && n > 64 ? (size_t)OBS_WAVES * n * sizeof(uint32_t) : 0);' in src
    return lambda n, with_key_rows: n * const['OBS_WORDS'] * 4 + (const['OBS_BLOCK'] // 64 * n * 4 if with_key_rows and n > 64 else 0)


@pytest.fixture(scope='module')
def kernel():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert 'neighbors_kernel' in table, 'libtdship.so holds no neighbors_kernel'
    return table['neighbors_kernel']


def test_the_neighbor_kernel_needs_no_stack(kernel):
    """nothing in it needs scratch: no spills, no private arrays (the keys of a large scene live in LDS, not in a per-thread array)"""
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel


def test_the_neighbor_kernel_keeps_its_occupancy(kernel):
    """the bounds DESIGN.md 5.5g states: 36 VGPRs in this build, held at <= 64 -- eight waves per SIMD --, at most 104 SGPRs, wave64, workgroups
    of 256, no static LDS"""
    assert kernel['vgpr_count'] <= 64 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] == 8, kernel
    assert kernel['sgpr_count'] <= 104, kernel
    assert kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64 and kernel['group_segment_fixed_size'] == 0, kernel


def test_the_dynamic_lds_of_a_launch_is_what_the_design_states():
    """32 bytes per entity, and above 64 entities a row of 4-byte keys per wave: 2 KiB for the workload's 64 entities, 48 KiB at the limit of
    TDS_NEIGHBORS_MAX_ENTITIES -- within the 64 KiB a launch gets without asking for more.  Read from the constants the launch is sized by
    (csrc/tds_observers.h), with the key rows."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'neighbors.hip')).read()
    lds = frame()
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    limit = int(re.search(r'#define TDS_NEIGHBORS_MAX_ENTITIES (\d+)', header).group(1))
    assert limit == 1024 and 'tds::slice_grid(B, A), dim3(tds::OBS_BLOCK), tds::lds_bytes(E, true)' in src and 'TDS_NEIGHBORS_MAX_ENTITIES' in src
    assert lds(64, True) == 2 * 1024 and lds(65, True) == 65 * 48 and lds(limit, True) == 48 * 1024 <= 64 * 1024
