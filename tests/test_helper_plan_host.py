"""
The rule for the helper enqueue of the persistent raster launch (torchdrivesim_amd/csrc/tds_raster_plan.h: RasterPlan::helper_grid) compiled for
the HOST by tests/helper_plan_host.cpp and swept there over the shapes of tests/raster_plan_host.cpp: helper_grid > 0 only for a persistent
fused bit-plane plan of a colour image in 4-wave workgroups at three per CU, with queues, without index slices, with at least threshold x grid
work items -- and then it is three workgroups per CU of the helper stream; the rest of the plan never depends on the helper stream.  Built plain
and with the address and undefined-behaviour sanitizers and run as it is; nothing is loaded into Python.  CPU only.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'helper_plan_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def run(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope='module')
def output():
    return run(build('helper_plan_host'))


def test_the_helper_goes_only_to_long_persistent_colour_launches(output):
    print(output)
    assert 'FAILED' not in output
    plans, helped = (int(v) for v in output.splitlines()[0].split()[1::2])
    assert plans == 523 * 17 * 4 * 3 * 2 * 5 * 2 * 4        # (two mask modes, uint8, float32 without and with slices) = 5
    assert 0 < helped < plans


def test_the_headline_launch_takes_96_workgroups_and_a_short_one_none(output):
    """65 536 cameras at 256 x 256 on 224 CUs: 672 workgroups and 3 x 32 on the helper's CUs; 32 cameras (one item per workgroup, below the
    product's threshold of 4): none; 128 x 128 (the split form, form 1): none"""
    assert output.splitlines()[-3:] == ['cameras 65536 grid 672 helper_grid 96', 'cameras 32 grid 32 helper_grid 0', '128 px form 1 helper_grid 0']


def test_clean_under_the_sanitizers(output):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    program = build('helper_plan_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan')
    assert run(program) == output
