"""
The on-lane row rule of the persistent K3 bit-plane kernel for SMALL faces (raster.hip: process_small_bits<ROWS>, taken by drain_bits for
faces with all vertices inside the image and at most ROWS = TDS_RASTER_SMALL_ROWS rows) as sequential C (tests/small_rows_model.c), held
to the oracle's cv::fillConvexPoly restatement triangle by triangle.  CPU only; the kernel itself is compared with the oracle under -m gpu
(tests/test_gpu_small_faces.py).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'small_rows_model.c')
OUT = os.path.join(ROOT, 'tests', '_build', 'small_rows_model')
ROWS = int(re.search(r'#define TDS_RASTER_SMALL_ROWS (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))


@pytest.fixture(scope='module')
def model(oracle):
    libdir = os.path.join(ROOT, 'oracle', '_build')
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.run(['gcc', '-O2', '-Wall', '-o', OUT, SRC, '-L', libdir, '-ltds_oracle', f'-Wl,-rpath,{libdir}'], check=True)
    return OUT


def run(model, *args):
    return subprocess.run([model, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_the_kernel_takes_seven_rows():
    # the 7 x 7 grid below is every face of at most ROWS rows only while ROWS is 7
    assert ROWS == 7


@pytest.mark.parametrize('offset', [4, 0, 9])
def test_every_triangle_of_a_7x7_grid(model, offset):
    # all 7^6 vertex triples of a 7 x 7 grid inside a 16 x 16 image (in its middle, in its top-left and in its bottom-right corner): every
    # vertex order, every flat and degenerate configuration of up to seven rows; every one is small, none is skipped
    r = run(model, ROWS, 'exhaustive', 16, offset, 7)
    assert r.returncode == 0 and '117649 triangles, 0 differ, 0 not small' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('seed', [21, 22])
def test_random_small_triangles_at_256(model, seed):
    # up to seven rows and any width (x-major slivers across the whole image, faces of a few pixels, faces on the border)
    r = run(model, ROWS, 'random', 256, 4000, seed)
    assert r.returncode == 0 and '4000 triangles, 0 differ, 0 not small' in r.stdout, r.stdout + r.stderr


def test_the_check_can_fail(model):
    # without the bias the tie rows of y-major edges and the integer half-row positions of x-major edges go wrong, and a rule for one row
    # fewer leaves the seventh row's faces to nobody: the harness must say so both times
    r = run(model, ROWS, 'nobias-exhaustive', 16, 4, 7)
    assert r.returncode == 1 and ' 0 differ' not in r.stdout
    r = run(model, ROWS - 1, 'exhaustive', 16, 4, 7)
    assert r.returncode == 1 and ' 0 not small' not in r.stdout
