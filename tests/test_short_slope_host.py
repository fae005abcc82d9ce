"""
The rasteriser's edge slopes (torchdrivesim_amd/csrc/tds_short_slope.h) compiled for the HOST by tests/short_slope_host.cpp and held to
OpenCV's statement in 64-bit integers, ((xe - xs) << 17) + dy) / (2 dy): the short form for the edges of small faces on its whole domain
(every dy in 1 .. 6, every dx the packed coordinates allow, the reciprocal exact and one ulp off either way), the general form -- moved into
the header unchanged -- on the same domain and on a seeded sample with dy up to 255 and beyond.  The program is also built with the address and
undefined-behaviour sanitizers and run as it is.  CPU only; the kernel that uses the short form is compared with the oracle under -m gpu
(tests/test_gpu_small_block.py).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'short_slope_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
HEADER = open(os.path.join(INC, 'tds_short_slope.h')).read()
MAX_DY = int(re.search(r'#define TDS_SHORT_SLOPE_MAX_DY (\d+)', HEADER).group(1))
MAX_DX = int(re.search(r'#define TDS_SHORT_SLOPE_MAX_DX (\d+)', HEADER).group(1))
SAMPLES = 200000


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def run(program, *args):
    return subprocess.run([program, *map(str, args)], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope='module')
def program():
    return build('short_slope_host')


def test_the_domain_covers_the_kernels_that_use_it():
    # every edge of a face of at most TDS_RASTER_SMALL_ROWS rows (the persistent kernel's 7, the list rasteriser's 4) spans at most MAX_DY
    # rows, and every difference of two packed coordinates below COORD_LIMIT lies inside MAX_DX
    rows = int(re.search(r'#define TDS_RASTER_SMALL_ROWS (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))
    limit = int(re.search(r'constexpr int COORD_LIMIT = (\d+);', open(os.path.join(INC, 'raster.hip')).read()).group(1))
    assert rows - 1 <= MAX_DY == 6
    assert 2 * limit <= MAX_DX == 32767


def test_every_case_of_the_short_form_and_a_sample_of_the_general_one(program):
    r = run(program, SAMPLES)
    n_short = MAX_DY * (2 * MAX_DX + 1)
    assert n_short < 400000
    assert r.returncode == 0, r.stdout + r.stderr
    assert f'short {n_short} cases, 0 differ' in r.stdout, r.stdout + r.stderr
    assert f'general {n_short + SAMPLES} cases, 0 differ' in r.stdout, r.stdout + r.stderr


def test_the_check_can_fail(program):
    # a reciprocal 64 ulp off is outside what the short form's margins take: the program must say so
    r = run(program, 10, 1)
    assert r.returncode == 1 and 'short form differs' in r.stderr and ', 0 differ\ngeneral' not in r.stdout


def test_clean_under_the_sanitizers(program):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    san = build('short_slope_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    assert run(san, SAMPLES).stdout == run(program, SAMPLES).stdout
    assert run(san, SAMPLES).returncode == 0
