"""The registers, LDS and scratch the range-scan kernel ends at (DESIGN.md "K5"), asserted on the BUILT product: tools/kernel_resources.py
reads the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
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
    assert 'range_scan_kernel' in table, 'libtdship.so holds no range_scan_kernel'
    return table['range_scan_kernel']


def test_the_scan_kernel_needs_no_stack(kernel):
    """nothing in it needs scratch: no spills, no private arrays"""
    assert kernel['private_segment_fixed_size'] == 0 and kernel['vgpr_spill_count'] == 0 and kernel['sgpr_spill_count'] == 0, kernel


def test_the_scan_kernel_keeps_its_occupancy(kernel):
    """the bounds DESIGN.md 5.5b states: at most 72 VGPRs -- seven waves per SIMD --, at most 104 SGPRs, workgroups of 256, 16 bytes of static LDS"""
    assert kernel['vgpr_count'] <= 72 and kernel['agpr_count'] == 0 and kernel['waves_per_simd'] >= 7, kernel
    assert kernel['sgpr_count'] <= 104, kernel
    assert kernel['max_flat_workgroup_size'] == 256 and kernel['wavefront_size'] == 64 and kernel['group_segment_fixed_size'] <= 16, kernel


def test_the_dynamic_lds_of_a_launch_is_what_the_design_states():
    """32 bytes per entity + PEND x 256 x 8 bytes of waiting faces: 2 KiB + 16 KiB for 64 entities, 48 KiB at the limit of
    TDS_SCAN_MAX_ENTITIES -- within the 64 KiB a launch gets without asking for more.  Read from the constants the launch is sized by."""
    import re
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'scan.hip')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    limit = int(re.search(r'#define TDS_SCAN_MAX_ENTITIES (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))
    assert (const['SBLOCK'], const['PEND'], const['BOX_WORDS'], limit) == (256, 8, 8, 1024)
    lds = lambda E: E * const['BOX_WORDS'] * 4 + const['PEND'] * const['SBLOCK'] * 8
    assert lds(64) == 18 * 1024 and lds(limit) == 48 * 1024 <= 64 * 1024
