"""The registers, LDS and scratch the range-scan backward kernel ends at, asserted on the BUILT product: tools/kernel_resources.py
reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def kernels():
    """both instances: one map for every scene, one map per scene"""
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    found = {k: v for k, v in table.items() if k.startswith('range_scan_bwd_kernel')}
    assert sorted(found) == ['range_scan_bwd_kernel<false>', 'range_scan_bwd_kernel<true>'], sorted(found)
    return found


def test_the_kernel_needs_no_stack_and_spills_nothing(kernels):
    for name, k in kernels.items():
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)


def test_the_kernel_keeps_its_occupancy(kernels):
    """the bounds DESIGN.md 5.5p states: at most 128 VGPRs -- four waves per SIMD, more than the LDS of a scene lets in at the entity limit --,
    workgroups of 256, wave64, 256 bytes of static LDS (the workgroup-wide "any ray live" vote)"""
    for name, k in kernels.items():
        assert k['vgpr_count'] <= 128 and k['agpr_count'] == 0 and k['waves_per_simd'] >= 4, (name, k)
        assert k['sgpr_count'] <= 104, (name, k)
        assert k['max_flat_workgroup_size'] == 256 and k['wavefront_size'] == 64 and k['group_segment_fixed_size'] <= 256, (name, k)


def test_the_dynamic_lds_of_a_launch_is_what_the_design_states():
    """80 bytes per entity (32 staged, 48 of binary64 sums) + 16 KiB of ray records + 1 KiB of their entities: 22.4 KiB for 68 entities, 97 KiB at
    the limit of TDS_SCAN_MAX_ENTITIES -- beyond the 64 KiB a launch gets unasked, within the 160 KiB of a CU.  Read from the constants the launch
    is sized by."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'scan_bwd.hip')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    limit = int(re.search(r'#define TDS_SCAN_MAX_ENTITIES (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))
    assert (const['SGBLOCK'], const['SG_BOX_WORDS'], const['SG_ACC'], const['SG_REC'], limit) == (256, 8, 6, 8, 1024)
    lds = lambda E: (const['SG_ACC'] * E + const['SG_REC'] * const['SGBLOCK']) * 8 + const['SG_BOX_WORDS'] * E * 4 + const['SGBLOCK'] * 4
    assert lds(68) == 80 * 68 + 17 * 1024 and 64 * 1024 < lds(limit) == 97 * 1024 <= 160 * 1024
    assert 'hipFuncAttributeMaxDynamicSharedMemorySize' in src, 'the launch asks for what it needs beyond 64 KiB'
