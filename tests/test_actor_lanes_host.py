"""
How the rasteriser's actor wave deals a round's visible agents to its lanes (torchdrivesim_amd/csrc/tds_actor_lanes.h), compiled for the HOST by
tests/actor_lanes_host.cpp and held to a brute-force restatement: sets of 0, 1, 2, 20, 21, 22, 42, 43, 63 and 64 visible agents in fixed patterns
and a few hundred thousand random ones, for 1, 3, 63, 64, 65, 128 and 130 agents (one to three rounds of 64).  Over the producer steps of a round
every (visible agent, face) pair comes up on exactly one lane, nothing else does, lane 63 and the positions beyond the last visible agent hold
nothing.  The program is also built with the address and undefined-behaviour sanitizers and run as it is.  CPU only; the kernel that uses the
header is compared with the per-wave form and the oracle under -m gpu (tests/test_gpu_actor_wave.py).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'actor_lanes_host.cpp')
INC = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
BUILD = os.path.join(ROOT, 'tests', '_build')
SAMPLES = 300000
ROUNDS = sum((n + 63) // 64 for n in (1, 3, 63, 64, 65, 128, 130))
SETS = ROUNDS * (10 * 7 + SAMPLES // 8)


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.run(['g++', '-std=c++17', '-O2', '-Wall', '-Werror', *flags, '-I', INC, '-o', out, SRC], check=True)
    return out


def run(program, *args):
    return subprocess.run([program, *map(str, args)], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope='module')
def program():
    return build('actor_lanes_host')


def test_the_header_deals_what_the_kernel_has_lanes_for():
    header = open(os.path.join(INC, 'tds_actor_lanes.h')).read()
    faces, agents, rnd = (int(re.search(rf'#define {n} (\d+)', header).group(1)) for n in ('TDS_ACTOR_FACES', 'TDS_ACTOR_STEP_AGENTS', 'TDS_ACTOR_ROUND'))
    assert faces * agents == 63 and rnd == 64             # 63 lanes serve faces, lane 63 idles; a round is one lane per agent
    assert -(-rnd // agents) <= rnd                       # the step within a round fits below the round's first agent (scan_step keeps both in a0)


def test_every_pair_on_exactly_one_lane(program):
    r = run(program, SAMPLES)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f'actor lanes {SETS} sets, 0 differ' in r.stdout, r.stdout + r.stderr
    assert SETS > 300000


def test_the_check_can_fail(program):
    # a restatement that deals 20 agents per step disagrees with the header from 21 visible agents on: the program must say so
    r = run(program, 1000, 1)
    assert r.returncode == 1 and 'lane assignment differs' in r.stderr and ', 0 differ' not in r.stdout


def test_clean_under_the_sanitizers(program):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer linked in, run on its own: any report ends it with an error"""
    san = build('actor_lanes_host_san', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan')
    r = run(san, SAMPLES)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout == run(program, SAMPLES).stdout
