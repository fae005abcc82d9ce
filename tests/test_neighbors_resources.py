"""The registers, LDS and scratch the neighbour kernel ends at, asserted on the BUILT product: tools/kernel_resources.py reads
the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


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
    TDS_NEIGHBORS_MAX_ENTITIES -- within the 64 KiB a launch gets without asking for more.  Read from the constants the launch is sized by."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'neighbors.hip')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    limit = int(re.search(r'#define TDS_NEIGHBORS_MAX_ENTITIES (\d+)', header).group(1))
    assert (const['NB_BLOCK'], const['NB_AGENTS'], const['NB_WORDS'], limit) == (256, 16, 8, 1024)
    assert 'NB_WAVES = NB_BLOCK / 64' in src and '(E > 64 ? (size_t)NB_WAVES * E * sizeof(uint32_t) : 0)' in src
    lds = lambda E: E * const['NB_WORDS'] * 4 + (const['NB_BLOCK'] // 64 * E * 4 if E > 64 else 0)
    assert lds(64) == 2 * 1024 and lds(65) == 65 * 48 and lds(limit) == 48 * 1024 <= 64 * 1024
