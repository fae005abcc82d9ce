"""The registers, LDS and scratch the lane-observation kernel ends at, asserted on the BUILT product: tools/kernel_resources.py
reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
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
    assert 'lane_obs_kernel' in table, 'libtdship.so holds no lane_obs_kernel'
    return table['lane_obs_kernel']


def test_the_lane_observation_kernel_needs_no_stack(kernel):
    """nothing in it needs scratch: no spills, no private arrays (no (segment, u) per candidate is kept: a winner's foot is found again)"""
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel


def test_the_lane_observation_kernel_keeps_its_occupancy(kernel):
    """the bounds DESIGN.md 5.5i states: 60 VGPRs in this build, held at <= 64 -- eight waves per SIMD --, at most 104 SGPRs (68 in this build),
    wave64, workgroups of 256"""
    assert kernel['vgpr_count'] <= 64 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] == 8, kernel
    assert kernel['sgpr_count'] <= 104, kernel
    assert kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64, kernel


def test_the_lds_of_a_launch_is_what_the_design_states(kernel):
    """static: per wave the lanelet (4 bytes) and the foot's arc length (8 bytes) of at most 32 slots, 1536 bytes per workgroup; dynamic: nothing
    up to 64 lanelets, above that a row of 4-byte keys per wave -- 32 KiB at the limit of TDS_LANE_OBS_MAX_LANELETS, within the 64 KiB a launch
    gets without asking for more.  Read from the constants the launch is sized by."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'lane_obs.hip')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    limit = {k: int(v) for k, v in re.findall(r'#define TDS_LANE_OBS_(\w+) (\d+)', header)}
    assert const['LO_BLOCK'] == 256 and 'LO_WAVES = LO_BLOCK / 64' in src and 'LO_MAX_K = TDS_LANE_OBS_MAX_K' in src
    assert limit == dict(MAX_K=32, MAX_POINTS=32, MAX_HOPS=8, MAX_LANELETS=2048)
    waves = const['LO_BLOCK'] // 64
    assert kernel['group_segment_fixed_size'] == waves * limit['MAX_K'] * (4 + 8) == 1536
    assert 'g.key_stride = set->max_lanelets > 64 ? set->max_lanelets : 0;' in src
    assert '(size_t)LO_WAVES * g.key_stride * sizeof(uint32_t)' in src
    lds = lambda L: waves * L * 4 if L > 64 else 0
    assert lds(64) == 0 and lds(65) == 1040 and lds(limit['MAX_LANELETS']) + 1536 == 32 * 1024 + 1536 <= 64 * 1024
