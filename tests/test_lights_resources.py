"""The registers, LDS and scratch the traffic-light kernels end at, asserted on the BUILT product: tools/kernel_resources.py reads
the AMDGPU metadata of the code objects inside torchdrivesim_amd/lib/libtdship.so.  CPU suite: hipcc cross-compiles, no GPU involved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from test_neighbors_resources import frame  # noqa: E402
KERNELS = ('lights_step_kernel', 'lights_reset_kernel', 'stop_lines_kernel')


@pytest.fixture(scope='module')
def table():
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    table = kernel_resources.kernel_table(_native.LIB_PATH)
    for name in KERNELS:
        assert name in table, f'libtdship.so holds no {name}'
    return table


@pytest.mark.parametrize('name', KERNELS)
def test_no_kernel_needs_a_stack(table, name):
    """no spills and no private arrays: the clocks of a scene are two LDS rows, the keys of a scene with many lines live in LDS"""
    k = table[name]
    assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k


@pytest.mark.parametrize('name', KERNELS)
def test_the_kernels_keep_their_occupancy(table, name):
    """the bounds DESIGN.md 5.5h states: 18, 15 and 42 VGPRs in this build, held at <= 64 -- eight waves per SIMD --, at most 104 SGPRs, wave64,
    workgroups of 256"""
    k = table[name]
    assert k['vgpr_count'] <= 64 and k['agpr_count'] == 0 and k['waves_per_simd'] == 8, k
    assert k['sgpr_count'] <= 104 and k['max_flat_workgroup_size'] == 256 and k['wavefront_size'] == 64, k


def test_the_lds_is_what_the_design_states(table):
    """the step kernel: an int32 phase and a float32 remaining time per machine, 2 KiB for TDS_LIGHTS_MAX_MACHINES, static; the stop lines: 32 bytes
    per line, and above 64 lines a row of 4-byte keys per wave -- 48 KiB at the limit of TDS_LIGHTS_MAX_LIGHTS, within the 64 KiB a launch gets
    without asking for more.  Read from the constants the launches are sized by (the stop lines': csrc/tds_observers.h, with the key rows)."""
    src = open(os.path.join(ROOT, 'torchdrivesim_amd', 'csrc', 'lights.hip')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', src)}
    header = open(os.path.join(ROOT, 'include', 'tdship.h')).read()
    limit = {k: int(v) for k, v in re.findall(r'#define TDS_LIGHTS_MAX_(\w+) (\d+)', header)}
    assert limit == dict(MACHINES=256, PHASES=64, LIGHTS=1024, SKIPS=1024)
    assert const['LT_BLOCK'] == limit['MACHINES'] and table['lights_step_kernel']['group_segment_fixed_size'] == 8 * limit['MACHINES']
    assert table['lights_reset_kernel']['group_segment_fixed_size'] == 0 and table['stop_lines_kernel']['group_segment_fixed_size'] == 0
    lds = frame()
    assert 'tds::slice_grid(B, A), dim3(tds::OBS_BLOCK), tds::lds_bytes(N, true)' in src and 'TDS_LIGHTS_MAX_LIGHTS' in src
    assert lds(36, True) == 1152 and lds(64, True) == 2 * 1024 and lds(65, True) == 65 * 48 and lds(limit['LIGHTS'], True) == 48 * 1024 <= 64 * 1024
