"""
The block that paints a SMALL face on the lane that scanned it (raster.hip: process_small_bits<ROWS>, ROWS > 2: the persistent kernel's 7 rows,
the list rasteriser's 4) in the form it has with division-free slopes and one form for the rows between the vertices, as sequential C++
(tests/small_block_model.cpp, the row rule and the slopes from the kernel's own tds_face_rows.h and tds_short_slope.h), held to the oracle's
cv::fillConvexPoly restatement triangle by triangle: the exhaustive 7 x 7 vertex grid, flat wide faces of every height, middle row, width and
edge direction, random small faces; once more under the address and undefined-behaviour sanitizers.  CPU only; the kernel itself is compared with the oracle under -m gpu (tests/test_gpu_small_block.py).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'small_block_model.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
OUT = os.path.join(ROOT, 'tests', '_build', 'small_block_model')
ROWS = int(re.search(r'#define TDS_RASTER_SMALL_ROWS (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))
LIST_ROWS = 4                    # the list rasteriser's instantiation (raster.hip: process_small_bits<4>)


def build(out, *flags):
    libdir = os.path.join(ROOT, 'oracle', '_build')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC, '-L', libdir, '-ltds_oracle',
                    f'-Wl,-rpath,{libdir}'], check=True)
    return out


@pytest.fixture(scope='module')
def model(oracle):
    return build(OUT)


def run(model, *args):
    return subprocess.run([model, *map(str, args)], capture_output=True, text=True, timeout=600)


def wide_count(rows, res):
    # heights 1 .. rows - 1, the middle vertex in each of the h + 1 rows, widths 8 .. res - 1, 6 placements, 6 vertex orders
    return sum(h + 1 for h in range(1, rows)) * (res - 8) * 36


def test_the_kernels_take_seven_and_four_rows():
    assert ROWS == 7
    assert 'process_small_bits<4>' in open(os.path.join(INC, 'raster.hip')).read()


@pytest.mark.parametrize('offset', [4, 0, 9])
def test_every_triangle_of_a_7x7_grid(model, offset):
    # all 7^6 vertex triples of a 7 x 7 grid inside a 16 x 16 image (in its middle, in its top-left and in its bottom-right corner)
    r = run(model, ROWS, 'exhaustive', 16, offset, 7)
    assert r.returncode == 0 and '117649 triangles, 0 differ, 0 not small' in r.stdout, r.stdout + r.stderr


def test_every_triangle_of_a_4x4_grid_with_four_rows(model):
    r = run(model, LIST_ROWS, 'exhaustive', 16, 5, 4)
    assert r.returncode == 0 and '4096 triangles, 0 differ, 0 not small' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('rows,res', [(ROWS, 256), (ROWS, 512), (LIST_ROWS, 128)])
def test_flat_wide_faces(model, rows, res):
    # what no real map holds and the short slope could get wrong: 2 .. rows rows, 8 .. res - 1 pixels wide
    r = run(model, rows, 'wide', res)
    assert r.returncode == 0 and f'{wide_count(rows, res)} triangles, 0 differ, 0 not small' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('rows,res,seed', [(ROWS, 256, 31), (ROWS, 1024, 32), (LIST_ROWS, 128, 33)])
def test_random_small_triangles(model, rows, res, seed):
    r = run(model, rows, 'random', res, 4000, seed)
    assert r.returncode == 0 and '4000 triangles, 0 differ, 0 not small' in r.stdout, r.stdout + r.stderr


def test_the_check_can_fail(model):
    # the middle vertex's row painted as a row of part 1 misses the pixels of the edges that end and start there, and a rule for one row
    # fewer leaves the seventh row's faces to nobody: the harness must say so both times
    r = run(model, ROWS, 'oldrows-exhaustive', 16, 4, 7)
    assert r.returncode == 1 and ' 0 differ' not in r.stdout
    r = run(model, ROWS - 1, 'exhaustive', 16, 4, 7)
    assert r.returncode == 1 and ' 0 not small' not in r.stdout


def test_clean_under_the_sanitizers(model):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in (the oracle library as it is), run on its own: any report
    ends it with an error.  The chain products that may wrap stay in unsigned types, so there is nothing for it to say."""
    san = build(OUT + '_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    for args in [(ROWS, 'exhaustive', 16, 4, 7), (LIST_ROWS, 'exhaustive', 16, 5, 4)]:
        r = run(san, *args)
        assert r.returncode == 0 and r.stderr == '', r.stdout + r.stderr
        assert r.stdout == run(model, *args).stdout and ' 0 differ, 0 not small' in r.stdout
