"""
Heuristic scene initialisation (reference torchdrivesim/behavior/heuristic.py): agents standing on lanes, facing along them, not
overlapping.  The reference draws a random point on a random lanelet's centre line and rejects it when its 5-disc footprint touches an
agent placed earlier (inflated by a 1 m / 0.2 m gap), up to 500 attempts per agent -- one torch call and one Lanelet2 query per attempt,
for one scene.  Here a batch of scenes is ONE kernel launch (csrc/spawn.hip, `tds_spawn_on_lanes_f32`): the candidates come from a
counter-based random stream (Philox4x32-10 keyed by `seed`, counted by scene id, agent and attempt), so a scene's result depends on
`(seed, scene id)` only -- not on the batch it sits in -- and the launch can be captured into a HIP graph.  DESIGN.md, "On-lane
initialisation", states the build-defined points (eligible lanelets, [sin, cos] from the direction's unit vector, the counter layout).
"""
import random
from typing import List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from torchdrivesim_amd import _native as nat
from torchdrivesim_amd import _ops
from torchdrivesim_amd.behavior.common import InitializationFailedError
from torchdrivesim_amd.lanelet2 import LaneletMap, group_lanelet_maps, lane_set_for  # noqa: F401  (group_lanelet_maps is part of this module's surface)

# heuristic.py:11-16
LENGTH, WIDTH, LR = 4.97, 2.04, 1.96
LONGITUDINAL_GAP, LATERAL_GAP = 1.0, 0.2


def _device(device) -> torch.device:
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('heuristic initialisation runs on an MI355X; no GPU is visible (no CPU fallback)')
        return torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'heuristic initialisation runs on an MI355X; got device {device} (no CPU fallback)')
    return device


def heuristic_initialize_batch(lanelet_maps, batch_size: int, agent_num: int, min_speed=0, max_speed=10, num_attempts_per_agent: int = 500, *,
                               seed: int, scene_ids: Optional[Tensor] = None, agent_attributes: Optional[Tensor] = None,
                               occupied: Optional[Tensor] = None, occupied_mask: Optional[Tensor] = None, on_failure: str = 'raise',
                               device=None) -> Tuple[Tensor, Tensor, Tensor]:
    """
    `heuristic_initialize` for `batch_size` scenes in one launch.

    Args:
        lanelet_maps: one `LaneletMap` for all scenes or a list of `batch_size` of them
        agent_num: agents per scene, placed in index order
        seed: key of the random stream; the same seed gives the same scenes, bit for bit
        scene_ids: (B,) int64, default arange(B): the identity of each scene in the random stream.  Rows computed alone with the ids they
            have in a larger batch equal the rows of that batch (shards, sub-batches, re-initialising some scenes).
        agent_attributes: (B, A, 3) [length, width, lr]; default the reference's constants 4.97 / 2.04 / 1.96
        occupied, occupied_mask: (B, M, 5) boxes [x, y, length, width, psi] that are already there and their (B, M) presence mask;
            treated like agents placed earlier: inflated by the gap and tested against every candidate
        on_failure: 'raise' reads the `placed` mask back (one synchronisation, after the launch) and raises `InitializationFailedError`
            naming the first scene and agent without a place; 'mask' returns without synchronising
    Returns:
        agent_attributes (B, A, 3), agent_states (B, A, 4) = [x, y, psi, speed], placed (B, A) bool.  In a scene where agent i finds no
        place, agents i .. are not placed (state rows zero) -- the reference stops there too.
    """
    if on_failure not in ('raise', 'mask'):
        raise ValueError(f"on_failure must be 'raise' or 'mask', got {on_failure!r}")
    B, A = int(batch_size), int(agent_num)
    for name, t in (('scene_ids', scene_ids), ('agent_attributes', agent_attributes), ('occupied', occupied), ('occupied_mask', occupied_mask)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f'{name}: heuristic initialisation runs on an MI355X; got a {t.device} tensor (no CPU fallback)')
    device = _device(device)
    if agent_attributes is None:
        agent_attributes = torch.empty((B, A, 3), dtype=torch.float32, device=device)       # three fills: nothing crosses from the host, so
        for k, v in enumerate((LENGTH, WIDTH, LR)):                                          # the call can be captured into a graph
            agent_attributes[..., k] = v
    elif tuple(agent_attributes.shape) != (B, A, 3):
        raise ValueError(f'agent_attributes must be ({B}, {A}, 3), got {tuple(agent_attributes.shape)}')
    if B == 0 or A == 0:
        return agent_attributes, torch.zeros((B, A, 4), dtype=torch.float32, device=device), torch.zeros((B, A), dtype=torch.bool, device=device)
    occupied_sc = None
    if occupied is not None:
        if occupied_mask is None:
            occupied_mask = torch.ones(occupied.shape[:2], dtype=torch.bool, device=occupied.device)
        inflated = occupied.to(torch.float32).clone()
        inflated[..., 2] += LONGITUDINAL_GAP
        inflated[..., 3] += LATERAL_GAP
        occupied_sc = _ops.metric_sc(inflated, 'discs')
    elif occupied_mask is not None:
        raise ValueError('occupied_mask without occupied')
    lane_set = lane_set_for(lanelet_maps, B, device)
    states, _, placed, _ = _ops.spawn_on_lanes(lane_set, scene_ids, agent_attributes, seed, min_speed, max_speed, (LONGITUDINAL_GAP, LATERAL_GAP),
                                               num_attempts_per_agent, occupied, occupied_sc, occupied_mask)
    if on_failure == 'raise':
        missing = (~placed).nonzero()
        if missing.shape[0] > 0:
            b, i = (int(v) for v in missing[0])
            raise InitializationFailedError(f'scene {b}: agent {i} found no free place on the lanes in {num_attempts_per_agent} attempts')
    return agent_attributes, states, placed


def heuristic_initialize(lanelet_map, agent_num: int, min_speed=0, max_speed=10, num_attempts_per_agent: int = 500, *, seed: Optional[int] = None,
                         device=None) -> Tuple[Tensor, Tensor]:
    """
    The reference's `heuristic_initialize` (heuristic.py:10-53): `(agent_attributes (1, A, 3) = [length, width, lr], agent_states (1, A, 4) =
    [x, y, psi, speed])`; raises `InitializationFailedError` when some agent finds no place.  `seed=None` draws one from Python's `random`,
    where the reference takes its randomness.  It is `heuristic_initialize_batch` with one scene.
    """
    if agent_num == 0:
        # the reference returns the two shapes SWAPPED for an empty scene (heuristic.py:53); kept, callers may rely on it
        return torch.zeros(1, 0, 4, device=device), torch.zeros(1, 0, 3, device=device)
    if seed is None:
        seed = random.getrandbits(64)
    attributes, states, _ = heuristic_initialize_batch(lanelet_map, 1, agent_num, min_speed, max_speed, num_attempts_per_agent, seed=seed,
                                                       on_failure='raise', device=device)
    return attributes, states
