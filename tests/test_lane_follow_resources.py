"""The registers, LDS and scratch the lane-following step kernel ends at, asserted on the BUILT product: tools/kernel_resources.py
reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def kernels():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert 'lane_follow_kernel' in table and 'lane_snap_kernel' in table, 'libtdship.so holds no lane-following kernels'
    return table


def test_the_step_kernel_needs_no_stack(kernels):
    """nothing in it needs scratch: no spills, no private arrays (the path lives in LDS)"""
    for name in ('lane_follow_kernel', 'lane_snap_kernel'):
        k = kernels[name]
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)


def test_the_step_kernel_keeps_its_occupancy(kernels):
    """the bounds DESIGN.md 5.5c states.  The occupancy the kernel relies on is set by its LDS: 51 KiB per four-wave workgroup at 64 entities =
    three workgroups per 160 KiB CU = three waves per SIMD.  The registers must leave that alone with one step to spare: at most 128 VGPRs = four
    waves per SIMD.  At most 104 SGPRs, workgroups of at most 256, no static LDS."""
    k = kernels['lane_follow_kernel']
    assert k['vgpr_count'] <= 128 and k['agpr_count'] == 0 and k['waves_per_simd'] >= 4, k
    assert k['sgpr_count'] <= 104, k
    assert k['max_flat_workgroup_size'] == 256 and k['wavefront_size'] == 64 and k['group_segment_fixed_size'] == 0, k


def test_the_dynamic_lds_of_a_launch_is_what_the_design_states():
    """32 bytes per entity + per wave 256 path pieces of 48 bytes and 64 ints for the entities in reach; four waves up to 480 entities (15 + 48 + 1
    KiB), two above (at most 32 + 24 + 0.5 KiB at TDS_FOLLOW_MAX_ENTITIES): within the 64 KiB a launch gets without asking for more.  Read from
    the constants the launch is sized by."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'follow.hip')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    limit = int(re.search(r'#define TDS_FOLLOW_MAX_ENTITIES (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))
    assert (const['FBLOCK'], const['FOLLOW_MAX_PIECES'], const['ENT_WORDS'], const['PIECE_DOUBLES'], const['NEAR_SLOTS'], limit) == (256, 256, 8, 6, 64, 1024)
    assert 'const int waves = E <= 480 ? 4 : 2;' in src
    lds = lambda E: E * const['ENT_WORDS'] * 4 + (4 if E <= 480 else 2) * (const['FOLLOW_MAX_PIECES'] * const['PIECE_DOUBLES'] * 8 + const['NEAR_SLOTS'] * 4)
    assert lds(64) == 51 * 1024 and lds(480) == 64 * 1024 and lds(481) < lds(limit) == 56 * 1024 + 512
    from torchdrivesim_amd import _native
    assert (_native.FOLLOW_MAX_ENTITIES, _native.FOLLOW_MAX_HOPS) == (limit, 8)
