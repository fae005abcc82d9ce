"""Host logic of the on-lane initialisation without a device: argument checks of the ABI, the Python layer's refusals and shapes, the
grouping of map lists, the rules spawn.hip is held to, and its resource guard."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT


def test_abi_argument_checks_are_loud_and_launch_nothing():
    from torchdrivesim_amd import _native
    L = _native.lib()

    def call(n_scenes=1, agents=1, n_occ=0, max_attempts=500, min_speed=0.0):
        return L.tds_spawn_on_lanes_f32(None, None, None, n_scenes, agents, None, None, None, None, n_occ, 1, min_speed, 10.0, 1.0, 0.2, max_attempts,
                                        None, None, None, None, None)
    for kw, word in ((dict(agents=-1), 'agents_per_scene'), (dict(max_attempts=0), 'max_attempts'), (dict(n_scenes=-1), 'n_scenes'),
                     (dict(n_occ=-1), 'n_occupied'), (dict(agents=2000, n_occ=49), 'LDS'), (dict(min_speed=float('nan')), 'finite'),
                     (dict(), 'lane-table set is null')):
        assert call(**kw) == _native.E_INVAL and word in _native.last_error(), (kw, _native.last_error())
    assert _native.SPAWN_MAX_BOXES == int(re.search(r'#define TDS_SPAWN_MAX_BOXES (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))


def test_cpu_tensors_and_cpu_devices_are_refused():
    from torchdrivesim_amd import _ops, lanelet2
    from torchdrivesim_amd.behavior import heuristic_initialize, heuristic_initialize_batch
    m = lanelet2.LaneletMap([], np.zeros((0, 3)), [lanelet2.make_lanelet(1, [(0, 1), (30, 1)], [(0, -1), (30, -1)])])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        heuristic_initialize_batch(m, 2, 3, seed=1, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        heuristic_initialize_batch(m, 2, 3, seed=1, agent_attributes=torch.ones(2, 3, 3), device='cuda:0')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        heuristic_initialize(m, 3, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _ops.spawn_on_lanes(None, None, torch.ones(2, 3, 3), 1)
    with pytest.raises(ValueError):
        heuristic_initialize_batch(m, 2, 3, seed=1, on_failure='ignore')


def test_no_agents_returns_the_references_swapped_shapes():
    """heuristic.py:53: `return torch.zeros(1, 0, 4), torch.zeros(1, 0, 3)` -- attributes and states trade places for an empty scene"""
    from torchdrivesim_amd.behavior import heuristic_initialize
    attributes, states = heuristic_initialize(None, 0)
    assert tuple(attributes.shape) == (1, 0, 4) and tuple(states.shape) == (1, 0, 3)


def test_a_list_of_maps_is_grouped_into_distinct_tables():
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.behavior.heuristic import group_lanelet_maps
    a, b = (lanelet2.LaneletMap([], np.zeros((0, 3)), []) for _ in range(2))
    assert group_lanelet_maps(a, 5) == ([a], None)
    assert group_lanelet_maps([a, a, a], 3) == ([a], None)
    uniq, scene_map = group_lanelet_maps([b, a, b, None, a], 5)
    assert uniq[0] is b and uniq[1] is a and len(uniq) == 2 and scene_map == [0, 1, 0, -1, 1]
    with pytest.raises(ValueError):
        group_lanelet_maps([a, b], 3)


def test_the_functions_are_exported():
    import torchdrivesim_amd.behavior as behavior
    assert {'heuristic_initialize', 'heuristic_initialize_batch', 'InitializationFailedError'} <= set(behavior.__all__)
    assert 'not provided' not in behavior.__doc__.split('IAI')[0]


def test_spawn_entry_point_neither_allocates_nor_synchronises():
    """the rule of tests/test_abi.py::test_no_per_call_entry_point_allocates_or_synchronises, held for spawn.hip and the header it shares with
    K2a; and no inline assembly anywhere in it"""
    csrc = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
    banned = ('hipMalloc', 'hipFree', 'hipMemset', 'hipMemcpy(', 'hipMemcpyAsync', 'hipStreamSynchronize', 'hipDeviceSynchronize', 'hipEventSynchronize',
              'hipHostMalloc', 'asm', '__syncthreads')
    for name in ('spawn.hip', 'tds_discs.h'):
        src = re.sub(r'//.*', '', open(os.path.join(csrc, name)).read())
        for word in banned:
            assert word not in src, f'{name} mentions {word}'


def test_disc_metric_has_one_definition():
    csrc = os.path.join(ROOT, 'torchdrivesim_amd', 'csrc')
    for name in ('collision.hip', 'spawn.hip'):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "tds_discs.h"' in src and 'float discs_pair(' not in src


def test_spawn_kernel_uses_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    e = kernel_resources.kernel_table(_native.LIB_PATH)['spawn_on_lanes_kernel']
    assert e['private_segment_fixed_size'] == 0 and e['vgpr_spill_count'] == 0, e
