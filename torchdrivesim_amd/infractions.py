"""
Infraction metrics with the reference's names and signatures (torchdrivesim/infractions.py), computed by the K2 HIP
kernels: oriented-box IoU, 5-disc overlap, and off-road distance to the driving-surface mesh.
"""
from typing import Optional, Union

import os
import numpy as np
import torch
from torch import Tensor

from torchdrivesim_amd import _ops
from torchdrivesim_amd.mesh import BaseMesh


def iou_differentiable(box1: Tensor, box2: Tensor, fast: bool = True) -> Tensor:
    """Approximate IoU of oriented boxes, element-wise over BxAx5 tensors [x,y,length,width,psi] (infractions.py:307-324,
    _iou_utils.py:344-367).  Forward only; `Simulator.compute_collision` is the differentiable entry point."""
    if not fast:
        raise NotImplementedError('only the fast Rotated-IoU variant exists (the reference imports the slow one from a private package)')
    return _ops.pairwise_overlap(box1, box2, 'iou')


def collision_detection_with_discs(box1: Tensor, box2: Tensor, num_discs: int = 5, backend: str = 'torch') -> Tensor:
    """TrafficSim-style overlap of `num_discs` discs per box, relu(1 - d / (r1 + r2)) (infractions.py:503-545); `num_discs` odd,
    3 .. 25 (torch.cdist, which the reference calls, changes its formulation above 25 points per set)."""
    assert isinstance(num_discs, int) and num_discs > 1 and num_discs % 2 != 0          # bbox2discs, infractions.py:391
    if backend != 'torch':
        raise ValueError('Unknown backend framework.')
    return _ops.pairwise_overlap(box1, box2, 'discs', num_discs=num_discs)


def box2corners_th(box: Tensor) -> Tensor:
    """(B,N,5) boxes -> (B,N,4,2) corners (_iou_utils.py:270-299)"""
    return _ops.box2corners(box)


#: grid cell (metres) of the geometry-only maps built for the off-road query: point location wants cells of about a face's size
#: (the rasteriser's own maps keep the library default, 8 m, which suits its row scans)
OFFROAD_CELL_SIZE = float(os.environ.get('TDS_OFFROAD_CELL', 3.0))


def _static_maps_for(mesh: BaseMesh, device) -> Union[_ops.StaticMap, _ops.StaticMapSet]:
    """The geometry-only device map of a batch of meshes (`_ops.map_per_distinct_row`: a StaticMap, or a StaticMapSet served in one launch
    when the batch holds several meshes), remembered on the mesh object."""
    key = (mesh.verts.data_ptr(), mesh.faces.data_ptr(), tuple(mesh.verts.shape), tuple(mesh.faces.shape), str(device))
    cache = getattr(mesh, '_tds_offroad_maps', None)
    if cache is not None and cache[0] == key:
        return cache[1]
    dev = torch.device(device)
    tensors = [t.detach() if t.is_cuda else t.detach().to(dev) for t in (mesh.verts, mesh.faces)]
    smap = _ops.map_per_distinct_row(tensors, lambda reps: (
        lambda h, rows: ('offroad', str(dev), h, tuple(tuple(x.shape) for x in rows), OFFROAD_CELL_SIZE),
        lambda r: _ops.StaticMap(tensors[0][r][..., :2], tensors[1][r], device=dev, cell_size=OFFROAD_CELL_SIZE)))
    try:
        object.__setattr__(mesh, '_tds_offroad_maps', (key, smap))
    except Exception:
        pass
    return smap


def offroad_infraction_loss(agent_states: Tensor, lenwid: Tensor, driving_surface_mesh: Union[BaseMesh, _ops.StaticMap],
                            threshold: float = 0, use_pytorch3d: Optional[bool] = None) -> Tensor:
    """Sum over the 4 agent corners of the thresholded SQUARED distance to the mesh (infractions.py:176-229, the pure
    torch path: `F.threshold(d, threshold, 0)` keeps d).  agent_states BxAx4, lenwid BxAx2 or Bx2 -> BxA."""
    if use_pytorch3d:
        raise NotImplementedError('pytorch3d is not part of this framework; the HIP kernel follows the pure-torch path')
    B, A = agent_states.shape[:2]
    if isinstance(driving_surface_mesh, _ops.StaticMap):
        smap, n_faces = driving_surface_mesh, driving_surface_mesh.n_faces
    else:
        smap, n_faces = None, driving_surface_mesh.faces_count
    if A == 0 or n_faces == 0:
        return torch.zeros_like(agent_states[..., 0])
    if lenwid.dim() == 2:
        lenwid = lenwid.unsqueeze(-2).expand((lenwid.shape[0], A, lenwid.shape[1]))
    if smap is None:
        smap = _static_maps_for(driving_surface_mesh, agent_states.device)
    return _ops.offroad(smap, agent_states, lenwid, threshold=threshold)


LANELET_TAGS_TO_EXCLUDE = ['parking']          # infractions.py:21


def lane_table_set(lanelet_maps, device, lanelet_dist_tolerance: float = 1.0) -> Optional[_ops.LaneTableSet]:
    """The device lane tables of a batch of maps (one table per DISTINCT map object, entries `None` -> no table)."""
    uniq, index = [], {}
    scene_map = []
    for m in lanelet_maps:
        if m is None:
            scene_map.append(-1)
            continue
        if id(m) not in index:
            index[id(m)] = len(uniq)
            uniq.append(m)
        scene_map.append(index[id(m)])
    if not uniq:
        return None
    tables = [m.table(device, LANELET_TAGS_TO_EXCLUDE, lanelet_dist_tolerance) for m in uniq]
    return _ops.LaneTableSet(tables, torch.tensor(scene_map, dtype=torch.int32))


def lanelet_orientation_loss(lanelet_maps, agents_state: Tensor, recenter_offset: Optional[Tensor] = None,
                             direction_angle_threshold: float = np.pi / 2, lanelet_dist_tolerance: float = 1.0,
                             lane_set: Optional[_ops.LaneTableSet] = None, differentiable: bool = False) -> Tensor:
    """
    Wrong-way loss (infractions.py:232-304): for every agent the lanelets within `lanelet_dist_tolerance` of its position, the
    local direction of each one's centre line, d = normalize_angle(direction - psi), loss = min over them of
    -cos(d) * [|d| > direction_angle_threshold]; 0 without such a lanelet, for scenes whose map is None, near a lanelet tagged
    'parking', and where the reference's `find_direction` raises.  One kernel launch for the batch (csrc/lanes.hip) instead of the
    reference's Python loop over scenes, agents and lanelets.  `lanelet_maps`: a list of B `torchdrivesim_amd.lanelet2.LaneletMap`
    or None; `lane_set`: the prepared tables of these maps (callers that query every step keep it).

    `differentiable=True`, with grad mode on and an `agents_state` that requires grad: the same values, bit for bit, and the result carries the
    graph to `agents_state[..., 2]` alone, as the reference's does (its position passes through float() and is a constant; psi stays a tensor):
    d loss / d psi = -sin(d) of the lanelet that attains the minimum where |d| exceeds the threshold, else 0 (`_ops.wrong_way_grad`, DESIGN.md
    5.5r).  x, y and the speed get exactly zero.  Otherwise nothing is recorded and nothing is saved.
    """
    assert len(lanelet_maps) == agents_state.shape[0]
    if recenter_offset is not None:
        assert len(lanelet_maps) == recenter_offset.shape[0]
    assert direction_angle_threshold >= np.pi / 2, 'direction_angle_threshold smaller than pi / 2 will produce false positives'
    if lane_set is None:
        lane_set = lane_table_set(lanelet_maps, agents_state.device, lanelet_dist_tolerance)
    if lane_set is None or agents_state.shape[1] == 0:
        return torch.zeros(agents_state.shape[:2], dtype=torch.float, device=agents_state.device)
    if differentiable and torch.is_grad_enabled() and agents_state.requires_grad:
        return _ops.wrong_way_grad(lane_set, agents_state, recenter_offset, None, direction_angle_threshold, lanelet_dist_tolerance)
    return _ops.wrong_way(lane_set, agents_state, recenter_offset, None, direction_angle_threshold, lanelet_dist_tolerance)
