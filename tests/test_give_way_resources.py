"""The registers, LDS and scratch the two kernels of giving way end at, asserted on the BUILT product: tools/kernel_resources.py reads
the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
KERNELS = ('lane_conflicts_kernel', 'lane_give_way_kernel')


@pytest.fixture(scope='module')
def kernels():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    assert all(k in table for k in KERNELS), 'libtdship.so holds no give-way kernels'
    return table


def test_the_kernels_need_no_stack(kernels):
    """no spills, no private arrays: the exclusions and the NPCs' summaries live in LDS"""
    for name in KERNELS:
        k = kernels[name]
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['agpr_count'] == 0 and k['wavefront_size'] == 64, (name, k)


def test_the_bounds_the_design_states(kernels):
    """the table kernel: workgroups of 256, one byte of LDS per lanelet of the largest table plus the four waves' zones; the yield pass: a
    workgroup of up to 1024 threads (16 waves = 4 per SIMD, so at most 128 VGPRs), no static LDS, 29 bytes of dynamic LDS per NPC"""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'conflicts.hip')).read()
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    lanelets, npcs = (int(re.search(rf'#define {name} (\d+)', header).group(1)) for name in ('TDS_CONFLICT_MAX_LANELETS', 'TDS_GIVE_WAY_MAX_NPCS'))
    assert (lanelets, npcs) == (2048, 1024)
    k = kernels['lane_conflicts_kernel']
    assert k['max_flat_workgroup_size'] == 256 and k['group_segment_fixed_size'] == lanelets + 2 * 4 * 8 and k['vgpr_count'] <= 128, k
    k = kernels['lane_give_way_kernel']
    assert k['max_flat_workgroup_size'] == npcs and k['group_segment_fixed_size'] == 0 and k['vgpr_count'] <= 128 and k['waves_per_simd'] >= 4, k
    assert 'constexpr int SUMMARY_BYTES = 3 * 8 + 4 + 1;' in src and '(size_t)block * SUMMARY_BYTES' in src
    assert npcs * 29 <= 64 * 1024, 'within what a launch gets without asking for more'
    from torchdrivesim_amd import _native
    import give_way_model
    assert (_native.CONFLICT_MAX_LANELETS, _native.GIVE_WAY_MAX_NPCS) == (lanelets, npcs) == (give_way_model.MAX_LANELETS, give_way_model.MAX_NPCS)
    assert {'tds_lane_conflicts_f64', 'tds_lane_give_way_multi', 'tds_lane_follow_step_stops_multi'} <= set(_native.DECLARATIONS)
    samples = int(re.search(r'constexpr int CONFLICT_MAX_SAMPLES = 1 << (\d+);', open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'tds_conflicts.h')).read()).group(1))
    assert 1 << samples == give_way_model.MAX_SAMPLES
