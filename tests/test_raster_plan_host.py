"""
The rasteriser's launch planning (torchdrivesim_amd/csrc/tds_raster_plan.h: the layouts of the caller's workspace, the shapes of the launches, the
byte counts of the sizing entry points) compiled for the HOST by tests/raster_plan_host.cpp and swept there: resolutions 1..520, 1024, 2048 and
4096; -1..15 keys; the four output modes; 1, 3, 64, 65 536 and 2^31 - 1 cameras; no workspace, 4096 bytes, the recommended size, four times that;
actor keys listed or not; index slices on and off; 32, 224 and 256 CUs.  The invariants are in the program (check_plan).  It is also built with the
address and undefined-behaviour sanitizers and run as it is; nothing is loaded into Python.  CPU only.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'raster_plan_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def run(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope='module')
def output():
    return run(build('raster_plan_host'))


def test_every_plan_of_the_sweep_keeps_its_invariants(output):
    print(output)
    assert 'FAILED' not in output
    plans = {line.split()[1]: int(line.split()[2]) for line in output.splitlines() if line.startswith('plans ')}
    assert sorted(plans) == ['binned', 'bits', 'error', 'fused', 'split'] and all(n > 0 for n in plans.values()), 'every form is among the plans'
    assert sum(plans.values()) == 523 * 17 * 5 * 4 * 2 * 3 * 5        # (two mask modes, uint8, float32 without and with slices) = 5


def test_the_binned_lists_of_the_smallest_call_end_inside_their_room(output):
    """one camera of one pixel in 4096 bytes: 4032 bytes of room, 256 of them the aligned counts -- 236 records, not the 250 of (4032 - 4) / 16
    less one (which ended at 4256)"""
    assert output.splitlines()[-1] == 'smallest form binned room 4032 lists 256 caps 236 end 4032'


def test_clean_under_the_sanitizers(output):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    program = build('raster_plan_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan')
    assert run(program) == output
