"""
`Simulator` facade with the reference's surface (torchdrivesim/simulator.py:280-1194): constructor injection of a
`KinematicModel` and a `BirdviewRenderer`, `TorchDriveConfig.collision_metric` dispatch, `step`, `render`,
`render_egocentric`, `compute_collision`, `compute_offroad`, `compute_wrong_way`, state accessors and the batch plumbing
(`copy`, `extend`, `select_batch_elements`, `to`).  Every hot call goes to a HIP kernel:

    step               -> K1 (kinematic.py)                                  reference: simulator.py:841-861
    render[_egocentric]-> K3 fused scene path (rendering/hip.py)             reference: simulator.py:920-1033
    compute_collision  -> K2a, all agents of all scenes in one launch        reference: simulator.py:1064-1194 (A launches)
    compute_offroad    -> K2b over the device-resident map grid              reference: simulator.py:1035-1044

    compute_neighbors  -> K6 (csrc/neighbors.hip), the K nearest entities per agent   reference: -- (get_all_agents_relative, all pairs)
    compute_stop_lines -> K7 (csrc/lights.hip), the K nearest stop lines per agent    reference: --
    compute_lanes      -> K8 (csrc/lane_obs.hip), the K nearest lanes per agent as polylines  reference: --
                          (differentiable=True: backward K8b, csrc/lane_obs_bwd.hip)
    compute_time_to_collision -> K9 (csrc/ttc.hip), when each agent would first touch another entity  reference: --
    compute_wrong_way  -> lane tables of `lanelet_map` (lanelet2.py), one launch  reference: simulator.py:607-630 (Python triple loop)

Also carried: traffic controls, waypoint goals (state + rendering), observation noise and lane features (plumbing only).  Out of scope
(SURVEY.md section 8): lanelet-derived lane features (the tensors are supplied by the caller).
"""
import logging
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, List, Optional

import numpy as np
import torch
from torch import Tensor

from torchdrivesim_amd import _ops
from torchdrivesim_amd.infractions import lane_table_set
from torchdrivesim_amd.kinematic import KinematicModel
from torchdrivesim_amd.mesh import BirdviewMesh, BirdviewRGBMeshGenerator, actor_template, set_colors_with_defaults
from torchdrivesim_amd.rendering import BirdviewRenderer, RendererConfig, renderer_from_config, HipRenderer
from torchdrivesim_amd.utils import Resolution, is_inside_polygon, relative, assert_equal

logger = logging.getLogger(__name__)


class CollisionMetric(Enum):
    """How collisions between agents are measured (simulator.py:27-34)."""
    iou = 'iou'                            #: approximate differentiable IoU of oriented rectangles
    discs = 'discs'                        #: differentiable overlap of rectangles approximated by 5 discs (default)
    nograd = 'nograd'                      #: number of other present agents whose rectangle overlaps (no gradient)
    nograd_pytorch3d = 'nograd-pytorch3d'  #: not available here


@dataclass
class TorchDriveConfig:
    """Top-level simulator configuration (simulator.py:37-51)."""
    renderer: RendererConfig = field(default_factory=lambda: RendererConfig())
    single_agent_rendering: bool = False
    collision_metric: CollisionMetric = field(default_factory=lambda: CollisionMetric.discs)
    offroad_threshold: float = 0.5
    left_handed_coordinates: bool = False
    wrong_way_angle_threshold: float = np.pi / 2
    lanelet_inclusion_tolerance: float = 1.0
    waypoint_removal_threshold: float = 2.0


@dataclass
class RangeScan:
    """What `Simulator.compute_range_scan` returns: three BxAxR tensors (metres, metres, int32 -- see there).  With
    `differentiable=True` `agents` and `road` carry the graph to the poses and sizes; `hit` never does."""
    agents: Tensor
    road: Tensor
    hit: Tensor


class _Slots:
    """What the per-observer top-K results share: `index` BxAxK int32 names the item of every slot, -1 for an empty one."""

    @property
    def mask(self) -> Tensor:
        """BxAxK bool: the slot is filled"""
        return self.index >= 0

    def take(self, per_item: Tensor, fill=0) -> Tensor:
        """Gathers a tensor BxNx... with a row per item of a scene -- per entity, Bx(A+Npc)x..., `get_all_agent_type()` and the like; per stop
        line, the control's `state`, `time_to_change`, ... -- at `index` -> BxAxKx..., `fill` in the empty slots."""
        B, A, K = self.index.shape
        if per_item.dim() < 2 or per_item.shape[0] != B:
            raise ValueError(f'take: expected a ({B}, E, ...) tensor, got {tuple(per_item.shape)}')
        rest = tuple(per_item.shape[2:])
        idx = self.index.clamp(min=0).to(torch.int64).reshape((B, A * K) + (1,) * len(rest)).expand((B, A * K) + rest)
        got = torch.gather(per_item, 1, idx).reshape((B, A, K) + rest)
        return torch.where(self.mask.reshape((B, A, K) + (1,) * len(rest)), got, torch.full((), fill, dtype=got.dtype, device=got.device))


@dataclass
class Neighbors(_Slots):
    """What `Simulator.compute_neighbors` returns: `features` BxAxKx8 float32 (the columns are `FEATURES`) and `index` BxAxK int32, the entity
    in [0, A + Npc) of every slot, -1 for an empty one (its features are all 0).  With `differentiable=True` `features` carries the graph to the
    poses, speeds and sizes it was computed from; `index` never does."""
    features: Tensor
    index: Tensor

    FEATURES = ('x', 'y', 'sin', 'cos', 'vx', 'vy', 'length', 'width')


@dataclass
class TimeToCollision(_Slots):
    """What `Simulator.compute_time_to_collision` returns: `ttc` BxAxK float32, the seconds until the agent first touches the entity of the slot
    (0: they overlap already), soonest first, +inf in an empty slot; `index` BxAxK int32, that entity in [0, A + Npc), -1 for an empty slot."""
    ttc: Tensor
    index: Tensor

    @property
    def min(self) -> Tensor:
        """BxA: the agent's time to its first collision, +inf if there is none within the horizon"""
        return self.ttc[..., 0]


@dataclass
class StopLines(_Slots):
    """What `Simulator.compute_stop_lines` returns: `features` BxAxKx8 float32 (the columns are `FEATURES`), `index` BxAxK int32, the stop line
    of every slot, and `state` BxAxK int32, its index into the control's `allowed_states`; -1 in both for an empty slot (its features are all 0:
    the state is kept out of them so that an empty slot cannot read as 'red' = 0)."""
    features: Tensor
    index: Tensor
    state: Tensor

    FEATURES = ('x', 'y', 'sin', 'cos', 'length', 'width', 'time_to_change', 'distance')


@dataclass
class Lanes(_Slots):
    """What `Simulator.compute_lanes` returns: `features` BxAxKx8 float32 (the columns are `FEATURES`), `points` BxAxKxPx2 float32, the centre
    line ahead of the foot in the agent's frame, `n_valid` BxAxK int32, how many of a slot's points are valid (the others are 0), and `index`
    BxAxK int32, the lanelet of every slot in its scene's `laneletLayer`, -1 for an empty one (its features and points are all 0).  From
    `compute_lanes(differentiable=True)` `features` and `points` can carry an autograd graph to the observing agent's pose; `n_valid` and `index`
    never do."""
    features: Tensor
    points: Tensor
    n_valid: Tensor
    index: Tensor

    FEATURES = ('x', 'y', 'sin', 'cos', 'arc', 'remaining', 'lateral', 'distance')

    @property
    def points_mask(self) -> Tensor:
        """BxAxKxP bool: the point is on the lane (the first `n_valid` of a slot are)"""
        return torch.arange(self.points.shape[-2], device=self.n_valid.device) < self.n_valid.unsqueeze(-1)


def _enlarge(x: Tensor, n: int) -> Tensor:
    return x.unsqueeze(1).expand((x.shape[0], n) + x.shape[1:]).reshape((n * x.shape[0],) + x.shape[1:])


class SpawnController:
    """Despawns NPCs that leave `exit_boundary` and spawns scheduled ones (simulator.py:54-124)."""

    def __init__(self, exit_boundary: Optional[Tensor] = None, spawn_states: Optional[Tensor] = None, spawn_masks: Optional[Tensor] = None):
        self.exit_boundary, self.spawn_states, self.spawn_masks = exit_boundary, spawn_states, spawn_masks
        self.time = 0

    def spawn_despawn_npcs(self, simulator: 'Simulator') -> None:
        ctrl = simulator.npc_controller
        mask, states = ctrl.npc_present_mask, ctrl.npc_state
        if self.exit_boundary is not None:
            mask = mask & is_inside_polygon(states[..., :2], self.exit_boundary)
        if self.spawn_states is not None and self.spawn_masks is not None:
            to_spawn = self.spawn_masks[..., self.time] & ~mask
            mask = mask | to_spawn
            states = self.spawn_states[..., self.time, :].where(to_spawn.unsqueeze(-1), states)
        ctrl.npc_present_mask, ctrl.npc_state = mask, states
        self.time += 1

    def _map(self, f):
        for k in ('exit_boundary', 'spawn_states', 'spawn_masks'):
            v = getattr(self, k)
            if v is not None:
                setattr(self, k, f(v))
        return self

    def to(self, device):
        return self._map(lambda x: x.to(device))

    def copy(self):
        return self.__class__(self.exit_boundary, self.spawn_states, self.spawn_masks)

    def extend(self, n, in_place=True):
        return (self if in_place else self.copy())._map(lambda x: _enlarge(x, n))

    def select_batch_elements(self, idx, in_place=True):
        return (self if in_place else self.copy())._map(lambda x: x[idx])


class NPCController:
    """Non-playable agents; the base class leaves them where they are (simulator.py:128-203)."""

    def __init__(self, npc_size: Tensor, npc_state: Tensor, npc_present_mask: Optional[Tensor] = None, npc_types: Optional[Tensor] = None,
                 agent_type_names: Optional[List[str]] = None, spawn_controller: Optional[SpawnController] = None):
        self.npc_size, self.npc_state = npc_size, npc_state
        self.npc_present_mask = npc_present_mask if npc_present_mask is not None else torch.ones_like(npc_state[..., 0], dtype=torch.bool)
        self.npc_types = npc_types if npc_types is not None else torch.zeros_like(self.npc_present_mask).long()
        self.agent_type_names = agent_type_names if agent_type_names is not None else ['vehicle']
        self.spawn_controller = spawn_controller if spawn_controller is not None else SpawnController()

    def get_npc_state(self):
        return self.npc_state

    def get_npc_size(self):
        return self.npc_size

    def get_npc_types(self):
        return self.npc_types

    def get_npc_present_mask(self):
        return self.npc_present_mask

    def spawn_despawn_npcs(self, simulator: 'Simulator') -> None:
        self.spawn_controller.spawn_despawn_npcs(simulator)

    def advance_npcs(self, simulator: 'Simulator') -> None:
        self.spawn_despawn_npcs(simulator)

    def _map(self, f):
        self.npc_size, self.npc_state = f(self.npc_size), f(self.npc_state)
        self.npc_present_mask, self.npc_types = f(self.npc_present_mask), f(self.npc_types)
        return self

    def to(self, device):
        self.spawn_controller.to(device)
        return self._map(lambda x: x.to(device))

    def copy(self):
        return self.__class__(self.npc_size, self.npc_state, self.npc_present_mask, self.npc_types, self.agent_type_names, self.spawn_controller.copy())

    def extend(self, n, in_place=True):
        me = self if in_place else self.copy()
        me.spawn_controller.extend(n, in_place=True)
        return me._map(lambda x: _enlarge(x, n))

    def select_batch_elements(self, idx, in_place=True):
        me = self if in_place else self.copy()
        me.spawn_controller.select_batch_elements(idx, in_place=True)
        return me._map(lambda x: x[idx])


class CompoundNPCController(NPCController):
    """
    Several NPC controllers over one set of NPCs: `controller_indices` (BxNpc) says which controller owns which NPC
    (simulator.py:206-278).  After every advance the owners' results are merged and the merged tensors handed back to ALL controllers,
    so that each of them sees the whole scene.  Deviation: `extend` repeats `controller_indices` per scene like every other tensor
    (the reference's `expand(n, -1)` only works for a batch of one).
    """

    def __init__(self, controllers: List[NPCController], controller_indices: Tensor):
        B, n = controller_indices.shape
        dev = controller_indices.device
        super().__init__(torch.zeros((B, n, 2), device=dev), torch.zeros((B, n, 4), device=dev), torch.zeros((B, n), device=dev, dtype=torch.bool),
                         None if controllers[0].npc_types is None else torch.zeros((B, n), device=dev, dtype=torch.long), controllers[0].agent_type_names)
        self.controllers = controllers
        self.controller_indices = controller_indices
        self.gather_npc_states()

    def gather_npc_states(self):
        for i, c in enumerate(self.controllers):
            mine = self.controller_indices == i
            self.npc_size = c.npc_size.where(mine.unsqueeze(-1), self.npc_size)
            self.npc_state = c.npc_state.where(mine.unsqueeze(-1), self.npc_state)
            self.npc_present_mask = c.npc_present_mask.where(mine, self.npc_present_mask)
            self.npc_types = c.npc_types.where(mine, self.npc_types)
        for c in self.controllers:
            c.npc_size, c.npc_state, c.npc_present_mask, c.npc_types = self.npc_size, self.npc_state, self.npc_present_mask, self.npc_types

    def advance_npcs(self, simulator: 'Simulator') -> None:
        for c in self.controllers:
            c.advance_npcs(simulator)
        self.gather_npc_states()

    def to(self, device):
        super().to(device)
        self.controller_indices = self.controller_indices.to(device)
        for c in self.controllers:
            c.to(device)
        return self

    def copy(self):
        return self.__class__([c.copy() for c in self.controllers], self.controller_indices.clone())

    def extend(self, n, in_place=True):
        me = self if in_place else self.copy()
        NPCController.extend(me, n, in_place=True)
        me.controller_indices = _enlarge(me.controller_indices, n)
        for c in me.controllers:
            c.extend(n, in_place=True)
        return me

    def select_batch_elements(self, idx, in_place=True):
        me = self if in_place else self.copy()
        NPCController.select_batch_elements(me, idx, in_place=True)
        me.controller_indices = me.controller_indices[idx]
        for c in me.controllers:
            c.select_batch_elements(idx, in_place=True)
        return me


class Simulator:
    """Batched 2-D driving simulator; see the module docstring.  Arguments follow simulator.py:283-309."""

    def __init__(self, road_mesh: BirdviewMesh, kinematic_model: KinematicModel, agent_size: Tensor, initial_present_mask: Tensor,
                 cfg: TorchDriveConfig, renderer: Optional[BirdviewRenderer] = None, lanelet_map=None, recenter_offset: Optional[Tensor] = None,
                 birdview_mesh_generator: Optional[BirdviewRGBMeshGenerator] = None, internal_time: int = 0, traffic_controls=None,
                 waypoint_goals=None, agent_types: Optional[Tensor] = None, agent_type_names: Optional[List[str]] = None,
                 npc_controller: Optional[NPCController] = None, agent_lr: Optional[Tensor] = None, lane_features=None,
                 observation_noise_model=None, action_model_extras: Optional[Dict[str, Any]] = None, route_goals=None):
        self._lane_set = None                            # device lane tables of `lanelet_map`, made on the first compute_wrong_way / compute_lanes
        self.road_mesh = road_mesh
        self.lanelet_map = lanelet_map
        self.recenter_offset = recenter_offset
        self.kinematic_model = kinematic_model
        self.agent_size = agent_size
        self.present_mask = initial_present_mask
        self.action_model_extras = action_model_extras
        self.traffic_controls = traffic_controls        # Dict[str, BaseTrafficControl]: state and violations; not rendered by the fused path
        self.waypoint_goals = waypoint_goals             # WaypointGoal: ticked off in step(), drawn as discs by render_egocentric
        self.route_goals = route_goals                   # goals.RouteGoal: one launch per step(); compute_route_progress() reports it
        self._route_progress = None                      # (state tensor, its version, RouteProgress) of the last route step
        self.lane_features = lane_features               # lanelet2.LaneFeatures: carried for policies, not used by any kernel
        if observation_noise_model is None:
            from torchdrivesim_amd.observation_noise import ObservationNoise
            observation_noise_model = ObservationNoise()
        self.observation_noise_model = observation_noise_model

        if not agent_type_names:
            agent_type_names = ['vehicle']
        if agent_types is None:
            agent_types = torch.zeros_like(initial_present_mask).long()
        if len(agent_types) == 1:
            agent_types = agent_types.expand_as(initial_present_mask)
        if agent_lr is None:
            agent_lr = torch.zeros_like(initial_present_mask).to(agent_size.dtype)
        if len(agent_lr) == 1:
            agent_lr = agent_lr.expand_as(initial_present_mask)
        self._agent_types = agent_type_names
        self._batch_size = self.road_mesh.batch_size
        self.agent_type = agent_types
        self.agent_lr = agent_lr

        self.npc_controller = npc_controller
        if self.npc_controller is None:
            dev = initial_present_mask.device
            self.npc_controller = NPCController(
                npc_size=torch.zeros((self._batch_size, 0, 2), dtype=self.agent_size.dtype, device=dev),
                npc_state=torch.zeros((self._batch_size, 0, 4), dtype=self.get_state().dtype, device=dev),
                npc_present_mask=torch.zeros((self._batch_size, 0), dtype=torch.bool, device=dev),
                npc_types=torch.zeros((self._batch_size, 0), dtype=torch.long, device=dev), agent_type_names=agent_type_names)
        self.validate_tensor_shapes()

        self.cfg: TorchDriveConfig = cfg
        if renderer is None:
            cfg.renderer.left_handed_coordinates = cfg.left_handed_coordinates
            self.renderer: BirdviewRenderer = renderer_from_config(cfg=cfg.renderer)
        else:
            self.renderer = renderer
        if cfg.left_handed_coordinates:
            self.kinematic_model.left_handed = cfg.left_handed_coordinates
        self.warned_no_lanelet = False
        self.internal_time = internal_time

        if birdview_mesh_generator is None:
            self.birdview_mesh_generator = BirdviewRGBMeshGenerator(background_mesh=self.road_mesh, color_map=self.renderer.color_map,
                                                                    rendering_levels=self.renderer.rendering_levels)
            self.birdview_mesh_generator.initialize_actors_mesh(self.get_all_agent_size(), self.get_all_agent_type(), self.agent_types)
        else:
            self.birdview_mesh_generator = birdview_mesh_generator
        if self.traffic_controls and getattr(self.birdview_mesh_generator, 'traffic_lights_mesh', None) is None:
            self.birdview_mesh_generator.initialize_traffic_controls_mesh(self.traffic_controls)      # simulator.py:373-374
        self._scene_cache = None        # device-resident static maps + actor templates/keys, rebuilt lazily
        self._fork = None               # (event, stamp, stream, results) recorded right before the last raster launch, see _beside_render
        self._fork_used = {}            # metrics asked for since then -> the grad mode they were asked in: enqueued ahead of the next raster launch

    # ------------------------------------------------------------------------------------------------- properties
    @property
    def agent_types(self) -> Optional[List[str]]:
        return self._agent_types

    @property
    def action_size(self) -> int:
        return self.kinematic_model.action_size

    @property
    def batch_size(self) -> int:
        return self._batch_size

    @property
    def agent_count(self) -> int:
        return self.get_agent_size().shape[-2]

    @property
    def npc_count(self) -> int:
        return self.get_npc_size().shape[-2]

    # ------------------------------------------------------------------------------------------------- plumbing
    def to(self, device):
        self.road_mesh = self.road_mesh.to(device)
        self.recenter_offset = self.recenter_offset.to(device) if self.recenter_offset is not None else None
        self.agent_size, self.agent_type = self.agent_size.to(device), self.agent_type.to(device)
        self.agent_lr, self.present_mask = self.agent_lr.to(device), self.present_mask.to(device)
        self.kinematic_model = self.kinematic_model.to(device)
        self.birdview_mesh_generator = self.birdview_mesh_generator.to(device)
        self.npc_controller = self.npc_controller.to(device)
        if self.traffic_controls is not None:
            self.traffic_controls = {k: v.to(device) for k, v in self.traffic_controls.items()}
        self.waypoint_goals = self.waypoint_goals.to(device) if self.waypoint_goals is not None else None
        self.route_goals = self.route_goals.to(device) if self.route_goals is not None else None
        self._route_progress = None
        self.lane_features = self.lane_features.to(device) if self.lane_features is not None else None
        self._scene_cache = None
        return self

    def copy(self):
        """Independent simulator sharing the tensors (shallow, simulator.py:421-442)."""
        other = self.__class__(
            road_mesh=self.road_mesh, kinematic_model=self.kinematic_model.copy(), agent_size=self.agent_size,
            initial_present_mask=self.present_mask, cfg=self.cfg, renderer=self.renderer.copy(), lanelet_map=self.lanelet_map,
            birdview_mesh_generator=self.birdview_mesh_generator.copy(), recenter_offset=self.recenter_offset, internal_time=self.internal_time,
            agent_types=self.agent_type, agent_type_names=self.agent_types, agent_lr=self.agent_lr, npc_controller=self.npc_controller.copy(),
            traffic_controls={k: v.copy() for k, v in self.traffic_controls.items()} if self.traffic_controls is not None else None,
            waypoint_goals=self.waypoint_goals.copy() if self.waypoint_goals is not None else None,
            observation_noise_model=self.observation_noise_model, lane_features=self.lane_features.copy() if self.lane_features is not None else None,
            route_goals=self.route_goals.copy() if self.route_goals is not None else None)
        other._scene_cache = self._scene_cache          # static maps are immutable and can be shared
        return other

    def extend(self, n: int, in_place: bool = True):
        if not in_place:
            other = self.copy()
            other.extend(n, in_place=True)
            return other
        self.road_mesh = self.road_mesh.expand(n)
        self.agent_size, self.agent_type = _enlarge(self.agent_size, n), _enlarge(self.agent_type, n)
        self.agent_lr, self.present_mask = _enlarge(self.agent_lr, n), _enlarge(self.present_mask, n)
        self.recenter_offset = _enlarge(self.recenter_offset, n) if self.recenter_offset is not None else None
        self.lanelet_map = [m for m in self.lanelet_map for _ in range(n)] if self.lanelet_map is not None else None
        self._lane_set = None
        self.lane_features = self.lane_features.extend(n) if self.lane_features is not None else None
        self.kinematic_model.extend(n)
        self._batch_size *= n
        self.birdview_mesh_generator = self.birdview_mesh_generator.expand(n)
        self.npc_controller = self.npc_controller.extend(n)
        if self.traffic_controls is not None:
            self.traffic_controls = {k: v.extend(n) for k, v in self.traffic_controls.items()}
        if self.waypoint_goals is not None:
            self.waypoint_goals = self.waypoint_goals.extend(n)
        if self.route_goals is not None:
            self.route_goals = self.route_goals.extend(n)
            self._route_progress = None
        self._scene_cache = None
        return self

    def select_batch_elements(self, idx, in_place=True):
        if not in_place:
            other = self.copy()
            other.select_batch_elements(idx, in_place=True)
            return other
        self.road_mesh = self.road_mesh[idx]
        self.recenter_offset = self.recenter_offset[idx] if self.recenter_offset is not None else None
        self.lanelet_map = [self.lanelet_map[i] for i in idx] if self.lanelet_map is not None else None
        self._lane_set = None
        self.lane_features = self.lane_features.select_batch_elements(idx) if self.lane_features is not None else None
        self.agent_size, self.agent_type = self.agent_size[idx], self.agent_type[idx]
        self.agent_lr, self.present_mask = self.agent_lr[idx], self.present_mask[idx]
        self.kinematic_model.select_batch_elements(idx)
        self._batch_size = len(idx)
        self.birdview_mesh_generator = self.birdview_mesh_generator.select_batch_elements(idx)
        self.npc_controller = self.npc_controller.select_batch_elements(idx)
        if self.traffic_controls is not None:
            self.traffic_controls = {k: v.select_batch_elements(idx) for k, v in self.traffic_controls.items()}
        if self.waypoint_goals is not None:
            self.waypoint_goals = self.waypoint_goals.select_batch_elements(idx)
        if self.route_goals is not None:
            self.route_goals = self.route_goals.select_batch_elements(idx)
            self._route_progress = None
        self._scene_cache = None
        return self

    def __getitem__(self, item):
        return self.select_batch_elements(item, in_place=False)

    def validate_agent_types(self):
        return

    def validate_tensor_shapes(self):
        assert_equal(len(self.kinematic_model.get_state().shape), 3)
        assert_equal(len(self.agent_size.shape), 3)
        assert_equal(len(self.agent_type.shape), 2)
        assert_equal(len(self.agent_lr.shape), 2)
        assert_equal(len(self.present_mask.shape), 2)
        b = self.batch_size
        for t in (self.kinematic_model.get_state(), self.agent_size, self.agent_type, self.agent_lr, self.present_mask):
            assert_equal(t.shape[0], b)
        assert_equal(self.road_mesh.batch_size, b)
        n = self.agent_count
        assert_equal(self.kinematic_model.get_state().shape[-2], n)
        assert_equal(self.agent_type.shape[-1], n)
        assert_equal(self.agent_lr.shape[-1], n)
        assert_equal(self.present_mask.shape[-1], n)

    # ------------------------------------------------------------------------------------------------- accessors
    def get_action_model_extras(self) -> Dict[str, Any]:
        return dict(self.action_model_extras) if self.action_model_extras else {}

    def get_world_center(self) -> Tensor:
        return self.birdview_mesh_generator.world_center

    def get_state(self) -> Tensor:
        return self.kinematic_model.get_state()

    def get_waypoints(self, count: int = 1):
        """B x A x count*M x 2 current waypoints of the agents, or None (simulator.py:589-593)"""
        return self.waypoint_goals.get_waypoints(count=count) if self.waypoint_goals is not None else None

    def get_waypoints_state(self):
        return self.waypoint_goals.state if self.waypoint_goals is not None else None

    def get_waypoints_mask(self, count: int = 1):
        return self.waypoint_goals.get_masks(count=count) if self.waypoint_goals is not None else None

    def get_agent_size(self) -> Tensor:
        return self.agent_size

    def get_agent_type(self) -> Tensor:
        return self.agent_type

    def get_agent_type_names(self) -> List[str]:
        return self._agent_types

    def get_agent_lr(self) -> Tensor:
        return self.agent_lr

    def get_present_mask(self) -> Tensor:
        return self.present_mask

    def get_npc_state(self) -> Tensor:
        return self.npc_controller.get_npc_state()

    def get_npc_size(self) -> Tensor:
        return self.npc_controller.get_npc_size()

    def get_npc_present_mask(self) -> Tensor:
        return self.npc_controller.get_npc_present_mask()

    def get_npc_types(self) -> Tensor:
        return self.npc_controller.get_npc_types()

    def get_all_agent_state(self) -> Tensor:
        return self.get_state() if self.npc_count == 0 else torch.cat([self.get_state(), self.get_npc_state()], dim=-2)

    def _heading_sc(self) -> Tensor:
        """[sin psi, cos psi] of ALL agents, computed once per state tensor and shared by render / collision / off-road (each of them
        would otherwise launch its own sin and cos); when gradients are being recorded, one shared autograd node.  The cache is keyed on the
        IDENTITY of the state tensor (which it keeps alive, so the allocator cannot hand its block to a later state) and on its
        version counter; a kinematic model whose get_state() builds a fresh tensor per call (CompoundKinematicModel) or a scene
        with NPCs (torch.cat per call) therefore never hits it."""
        state = self.get_all_agent_state()
        if state.requires_grad and torch.is_grad_enabled():
            # gradients are being recorded: ONE autograd node per state tensor (_ops.state_heading_sc), shared by render / collision / off-road
            # like the plain cache below -- autograd sums the three consumers' gradients before the node's closed-form backward runs once
            cached = getattr(self, '_sc_cache_grad', None)
            if cached is not None and cached[0] is state and cached[1] == state._version:
                return cached[2]
            sc = _ops.state_heading_sc(state)
            self._sc_cache_grad = (state, state._version, sc)
            return sc
        cached = getattr(self, '_sc_cache', None)
        if cached is not None and cached[0] is state and cached[1] == state._version:
            return cached[2]
        sc = _ops.heading_sc(state[..., 2].detach())
        self._sc_cache = (state, state._version, sc)
        return sc

    def get_all_agent_size(self) -> Tensor:
        return self.get_agent_size() if self.npc_count == 0 else torch.cat([self.get_agent_size(), self.get_npc_size()], dim=-2)

    def get_all_agent_present_mask(self) -> Tensor:
        return self.get_present_mask() if self.npc_count == 0 else torch.cat([self.get_present_mask(), self.get_npc_present_mask()], dim=-1)

    def get_all_agent_type(self) -> Tensor:
        return self.get_agent_type() if self.npc_count == 0 else torch.cat([self.get_agent_type(), self.get_npc_types()], dim=-1)

    def get_all_agents_absolute(self) -> Tensor:
        """Bx(A+Npc)x6: x, y, psi, length, width, present (simulator.py:730-738)."""
        return torch.cat([self.get_all_agent_state()[..., :3], self.get_all_agent_size(),
                          self.get_all_agent_present_mask().unsqueeze(-1).to(self.get_state().dtype)], dim=-1)

    def get_all_agents_relative(self, exclude_self: bool = True) -> Tensor:
        """BxAx(All[-1])x6: pose of every agent in the frame of each exposed agent (simulator.py:748-782); the diagonal is
        removed with a reshape trick instead of boolean indexing, so no device synchronisation is needed."""
        absolute = self.get_all_agents_absolute()
        A, total = self.agent_count, self.agent_count + self.npc_count
        xy, psi = absolute[..., :A, :2], absolute[..., :A, 2:3]
        rel_xy, rel_psi = relative(origin_xy=xy.unsqueeze(-2), origin_psi=psi.unsqueeze(-2), target_xy=absolute[..., :2].unsqueeze(-3),
                                   target_psi=absolute[..., 2:3].unsqueeze(-3))
        rel = torch.cat([rel_xy, rel_psi, absolute[..., 3:].unsqueeze(-3).expand(rel_xy.shape[:-1] + (3,))], dim=-1)
        if exclude_self:
            if A == 1:
                rel = rel[..., 1:, :]
            else:
                B = rel.shape[0]
                own, npc = rel[..., :A, :], rel[..., A:, :]
                # drop element (i, i) of an A x A block: flatten, skip every (A+1)-th entry
                own = own.reshape(B, A * A, 6)[:, 1:, :].reshape(B, A - 1, A + 1, 6)[:, :, :A, :].reshape(B, A, A - 1, 6)
                rel = torch.cat([own, npc], dim=-2)
                assert rel.shape[-2] == total - 1
        return rel

    # ---- what the exposed agents perceive (simulator.py:663-679, 740-746, 784-821)
    def get_noisy_state(self) -> Tensor:
        """BxAx(A+Npc)x4: the state of every agent as perceived by each exposed agent"""
        return self.observation_noise_model.get_noisy_state(self)

    def get_noisy_agent_size(self) -> Tensor:
        return self.observation_noise_model.get_noisy_agent_size(self)

    def get_noisy_present_mask(self) -> Tensor:
        return self.observation_noise_model.get_noisy_present_mask(self)

    def get_noisy_all_agents_absolute(self) -> Tensor:
        """BxAx(A+Npc)x6 [x, y, psi, length, width, present] in world coordinates, per observer"""
        return torch.cat([self.get_noisy_state()[..., :3], self.get_noisy_agent_size(), self.get_noisy_present_mask()[..., None]], dim=-1)

    def get_noisy_all_agents_relative(self, exclude_self: bool = True) -> Tensor:
        """BxAx(A+Npc [-1])x6 in the frame of each observer's OWN perceived pose; `exclude_self` drops the observer from its own list"""
        ab = self.get_noisy_all_agents_absolute()
        A, total = self.agent_count, self.agent_count + self.npc_count
        idx = torch.arange(A, device=ab.device)
        own = ab[:, idx, idx, :]
        rel_xy, rel_psi = relative(origin_xy=own[..., :2].unsqueeze(-2), origin_psi=own[..., 2:3].unsqueeze(-2), target_xy=ab[..., :2],
                                   target_psi=ab[..., 2:3])
        rel = torch.cat([rel_xy, rel_psi, ab[..., 3:]], dim=-1)
        if exclude_self:
            if A == 1:
                return rel[..., 1:, :]
            # drop column a of row a without boolean indexing (no device synchronisation): column j of the result is j + (j >= a)
            col = torch.arange(total - 1, device=ab.device)[None, :] + (torch.arange(total - 1, device=ab.device)[None, :] >= idx[:, None]).long()
            rel = torch.gather(rel, 2, col[None, :, :, None].expand(rel.shape[0], -1, -1, rel.shape[-1]))
        return rel

    def get_noisy_traffic_controls(self):
        return self.observation_noise_model.get_noisy_traffic_controls(self)

    def get_noisy_lane_features(self):
        return self.observation_noise_model.get_noisy_lane_features(self)

    def get_noisy_road_mesh(self):
        return self.observation_noise_model.get_noisy_road_mesh(self)

    def get_noisy_background_mesh(self):
        return self.observation_noise_model.get_noisy_background_mesh(self)

    def get_traffic_controls(self):
        return self.traffic_controls

    # ------------------------------------------------------------------------------------------------- dynamics
    def step(self, agent_action: Tensor) -> None:
        """One simulation step for BxAxAc actions (simulator.py:841-861)."""
        self.internal_time += 1
        assert_equal(len(agent_action.shape), 3)
        assert_equal(agent_action.shape[0], self.batch_size)
        assert_equal(agent_action.shape[-2], self.agent_count)
        self.npc_controller.advance_npcs(self)
        self._sc_cache_grad = None               # the shared [sin, cos] node of the state that is being left: do not pin its graph
        self._drop_fork()                        # nor do the metrics computed for it
        self.kinematic_model.step(agent_action)
        if self.traffic_controls is not None:                       # simulator.py:857-859
            for control in self.traffic_controls.values():
                control.step(self.internal_time)
        if self.waypoint_goals is not None:                         # simulator.py:860-861
            self.waypoint_goals.step(self.get_state(), self.internal_time, threshold=self.cfg.waypoint_removal_threshold)
        if self.route_goals is not None:
            self._step_route_goals()

    def _step_route_goals(self):
        state = self.get_state()
        # the [sin, cos] render / collision / off-road share for this state, where it covers exactly the exposed agents
        # (a differentiable goal gets the shared node itself: its gradient to psi joins those of render / collision / off-road there)
        sc = self._heading_sc() if self.npc_count == 0 and state.dtype == torch.float32 else None
        if sc is not None and not getattr(self.route_goals, 'differentiable', False):
            sc = sc.detach()
        out = self.route_goals.step(state, self.present_mask, sc=sc)
        self._route_progress = (state, state._version, out)
        return out

    def compute_route_progress(self):
        """The `goals.RouteProgress` of the current state (None without `route_goals`): the one `step` has made, or, after the state was set by
        other means since, one made now -- which, like every route step, moves the routes' cursors on and measures `advance` from the progress
        reported before it.  With `route_goals.differentiable` and a state that requires grad its float fields carry the graph to the state
        (`RouteGoal.step`); the price of the option is the six clones every such step makes of its output buffers."""
        if self.route_goals is None:
            return None
        state, cached = self.get_state(), self._route_progress
        if cached is not None and cached[0] is state and cached[1] == state._version:
            return cached[2]
        return self._step_route_goals()

    def set_state(self, agent_state: Tensor, mask: Optional[Tensor] = None) -> None:
        if mask is None:
            mask = torch.ones_like(agent_state[..., 0], dtype=torch.bool)
        assert_equal(len(agent_state.shape), 3)
        assert_equal(len(mask.shape), 2)
        assert_equal(agent_state.shape[0], self.batch_size)
        assert_equal(agent_state.shape[-2], self.agent_count)
        current = self.kinematic_model.get_state()
        k, full = agent_state.shape[-1], current.shape[-1]
        assert k <= full
        state = agent_state if k == full else torch.cat([agent_state, current[..., (k - full):]], dim=-1)
        self._sc_cache_grad = None
        self._drop_fork()
        self.kinematic_model.set_state(state.where(mask.unsqueeze(-1).expand_as(state), current))

    def update_present_mask(self, present_mask: Tensor) -> None:
        assert_equal(len(present_mask.shape), 2)
        assert_equal(present_mask.shape[0], self.batch_size)
        assert_equal(present_mask.shape[-1], self.agent_count)
        self.present_mask = present_mask

    def fit_action(self, future_state: Tensor, current_state: Optional[Tensor] = None) -> Tensor:
        return self.kinematic_model.fit_action(future_state=future_state, current_state=current_state)

    # ------------------------------------------------------------------------------------------------- infractions beside the rasteriser
    #: The GymEnv.step body (examples/gym_env.py:83-126 of the reference) is step -> render_egocentric -> compute_collision / compute_offroad /
    #: compute_wrong_way.  The rasteriser is bound by the HBM write stream and the metrics are compute-light and do not read the image, so they
    #: can run on a second HIP stream that waits only for what preceded the raster launch (an event, no host synchronisation) and is joined
    #: to the caller's stream before a result is handed out.  Same kernels, same inputs, same bits.
    #: The raster launch is PERSISTENT (its workgroups stay on their CUs until the last image is out), so metric kernels enqueued after it only
    #: get the slots they grab in the first microseconds (round 3: 7.51 ms per step beside, 7.30 behind).  Hence the metrics a loop asked for
    #: after its previous render are enqueued on the side stream right BEFORE the next raster launch, from inside `render` (`_mark_fork`):
    #: they take the CUs they need first, the surplus workgroups of the persistent launch start a few microseconds late and still find work,
    #: and `compute_*` hands the finished result out.  A metric that was not foreseen runs on the side stream after the launch, as in round 3,
    #: and is foreseen from then on; one that is no longer asked for is dropped after one step.  A metric is foreseen in the grad mode it was last
    #: ASKED FOR in (render() under no_grad for an observation, the infraction losses under grad: the foreseen result carries its graph), and what
    #: was computed for a state is let go when `step` / `set_state` leave that state.
    overlap_infractions = False
    _side_streams: Dict[int, Any] = {}
    _side_priority = -1          # HIP stream priority of the side stream (-1: high)
    #: overlap_infractions = 'reserved' (round 4): the raster launch runs on a stream that is kept off `_reserved_per_xcd` CUs per XCD, the metrics on a
    #: stream confined to exactly those (`_ops.reserved_streams`, hipExtStreamCreateWithCUMask).  The launch that stores every line is bound by the
    #: write stream and loses nothing on 224 of 256 CUs (tools/cu_mask_probe.hip); the launch of a loop that renders into a ring of owned buffers
    #: skips the background lines, is bound by instruction issue and DOES lose by them (4.9 ms alone on 256 CUs, 5.5 ms on 224: DESIGN.md section 6).
    #: So the metric stream is handed to the launch as its helper stream (`_ops.use_helper_cus`): once the metrics have ended -- about 1.3 of the
    #: 5 ms -- the reserved CUs run workgroups of the same launch.  The metrics lose nothing: they are enqueued first.
    _reserved_per_xcd = 4

    def _fork_sources(self):
        return [self.kinematic_model.get_state(), self.present_mask, self.agent_size, self.agent_type]

    def _side_stream(self, device):
        if self.overlap_infractions == 'reserved':
            return _ops.reserved_streams(device, Simulator._reserved_per_xcd)[1]          # confined to the CUs the raster launch is kept off
        idx = device.index if device.index is not None else torch.cuda.current_device()
        side = Simulator._side_streams.get(idx)
        if side is None:
            side = Simulator._side_streams[idx] = torch.cuda.Stream(device=device, priority=Simulator._side_priority)
        return side

    def raster_stream(self):
        """The stream that is kept off the reserved CUs (overlap_infractions = 'reserved'): a loop that runs under
        `with torch.cuda.stream(sim.raster_stream()):` renders on it without a detour, and its metrics run beside on the reserved CUs."""
        device = self.kinematic_model.get_state().device
        if not self._reserved_usable(device):
            return torch.cuda.current_stream(device)                # (warned once): the loop then simply runs on the caller's stream
        return _ops.reserved_streams(device, Simulator._reserved_per_xcd)[0]

    _reserved_warned = False

    def _reserved_usable(self, device) -> bool:
        """overlap_infractions = 'reserved' rests on what the bits of a CU mask stand for, which was OBSERVED on an MI355X in SPX mode
        (tools/cu_mask_probe.hip).  _ops.reserved_layout_ok launches a probe on both masked streams once per device and checks that the
        metric stream really runs on `_reserved_per_xcd` CUs of every XCD and the raster stream on all the others; on any other layout, or a
        device with fewer than 64 CUs (a CPX partition), the mode falls back to overlap_infractions = False with ONE warning -- it neither
        raises out of render() nor lets the "reserved" stream silently share the raster launch's CUs."""
        ok, why = _ops.reserved_layout_ok(device, Simulator._reserved_per_xcd) if device.type == 'cuda' else (False, 'not a GPU tensor')
        if not ok and not Simulator._reserved_warned:
            Simulator._reserved_warned = True
            import warnings
            warnings.warn(f"overlap_infractions='reserved' is not usable on {device} ({why}): the infraction metrics run behind the raster "
                          f"launch, as with overlap_infractions=False")
        return ok

    def _metric_fn(self, key):
        name = key[0]
        if name == 'collision':
            return lambda: self._compute_collision(None if key[1] is None else list(key[1]))
        return {'offroad': self._compute_offroad, 'wrong_way': self._compute_wrong_way}[name]

    def _mark_fork(self, write_bound: bool = True) -> None:
        """called by render() right before the raster launch: everything the metrics read has been enqueued by now.
        `write_bound`: the launch that follows is bound by the HBM write stream -- float32 images above 208 x 208.  (That is a statement about the
        BOUND, not about which kernel serves the launch: the fused persistent kernel starts above 160 x 160, raster.hip: split_serves, but a
        float32 launch between 160 and 208 pixels is still limited by instruction issue -- 192 x 192: 4.97 ms for 29 GB = 0.73 of the roof.)
        Only then does 'reserved' pay -- a compute-bound launch (uint8, low resolutions) would give an eighth of its CUs away for nothing, so
        the mode is skipped for it (the metrics run behind the launch)."""
        self._drop_fork()
        wanted, self._fork_used = getattr(self, '_fork_used', None) or {}, {}
        state = self.kinematic_model.get_state()
        if not self.overlap_infractions or not state.is_cuda or self.npc_count > 0:
            return
        if self.overlap_infractions == 'reserved' and (not write_bound or not self._reserved_usable(state.device)):
            return
        for grad_mode in {torch.is_grad_enabled(), *wanted.values()}:
            with torch.set_grad_enabled(grad_mode):
                self._heading_sc()                                # the shared [sin, cos] exists before the fork, in every grad mode it will be read in
        srcs = self._fork_sources()
        stream = torch.cuda.current_stream(state.device)
        ev = torch.cuda.Event()
        ev.record(stream)
        ready = {}
        if wanted:
            # the metrics of the previous step, ahead of the raster launch on the side stream
            side = self._side_stream(state.device)
            side.wait_event(ev)
            with torch.cuda.stream(side):
                for key, grad_mode in wanted.items():
                    with torch.set_grad_enabled(grad_mode):          # the mode compute_* was last called in, not the mode of this render
                        out = self._metric_fn(key)()
                    out.record_stream(stream)                        # allocated in the side stream's pool, consumed on the caller's stream
                    ready[key] = out
            done = torch.cuda.Event()
            done.record(side)
            ready = {k: (v, done, wanted[k]) for k, v in ready.items()}
        self._fork = (ev, [(t, t._version) for t in srcs], stream, ready)

    def _drop_fork(self) -> None:
        """Lets go of the last fork and of what was computed for it (step / set_state: the state it belongs to is being left, and a result
        that carries a graph would pin that step's autograd graph until the next render)."""
        prev, self._fork = self._fork, None
        if prev is not None:
            # a foreseen metric the loop did not ask for was never joined: its kernels read state / present / [sin, cos] that the
            # caller's stream is about to overwrite or free.  Join them here -- the launch they ran beside is long over, the wait is free
            # (and a captured graph has no dangling fork).
            for done in {id(entry[1]): entry[1] for entry in prev[3].values()}.values():
                prev[2].wait_event(done)

    def _beside_render(self, fn, key=None):
        """fn() -> Tensor: the result computed ahead of the raster launch when `key` was foreseen, else fn() on the side stream when a
        render of exactly this state is in flight on the current stream, else in place.
        With overlap_infractions on, asking for the same metric twice between two renders returns the SAME tensor object (the result is
        computed once per state) unless it carries a graph: treat the returned tensors as read-only, or clone them before an in-place edit.
        A result is handed out only in the grad mode it was computed in: one built under no_grad for a caller that records gradients is
        computed again, one that carries a graph is detached for a caller under no_grad, and a graph is handed out ONCE (asked for again,
        the metric is computed again -- a second backward() through a shared graph would find it freed), as in the serial order."""
        fork = self._fork
        if fork is None or not self.overlap_infractions:
            return fn()
        ev, stamp, main, ready = fork
        srcs = self._fork_sources()
        state = srcs[0]
        cached = getattr(self, '_sc_cache', None)
        if len(srcs) != len(stamp) or any(a is not b or a._version != v for a, (b, v) in zip(srcs, stamp)) or self.npc_count > 0 or \
                torch.cuda.current_stream(state.device) != main or cached is None or cached[0] is not state or cached[1] != state._version:
            return fn()
        grad_mode = torch.is_grad_enabled()
        if key is not None:
            self._fork_used[key] = grad_mode                         # foreseen at the next render, in this grad mode
        if key is not None and key in ready:
            out, done, built_with_grad = ready[key]
            main.wait_event(done)
            if out.requires_grad:
                if grad_mode:
                    del ready[key]                                   # a graph is handed out once
                    return out
                out = out.detach()
                ready[key] = (out, done, False)
                return out
            if built_with_grad or not grad_mode or not any(t.requires_grad for t in srcs):
                return out
            del ready[key]                                           # built under no_grad, wanted with its graph: computed again below
        side = self._side_stream(state.device)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            out = fn()
        out.record_stream(main)                                  # allocated in the side stream's pool, consumed on the caller's stream
        done = torch.cuda.Event()
        done.record(side)
        main.wait_event(done)
        if key is not None and not out.requires_grad:
            ready[key] = (out, done, grad_mode)                  # asked for again before the next render: the same tensor
        return out

    # ------------------------------------------------------------------------------------------------- device scene data
    def _scene(self):
        """Static maps (one per distinct road mesh in the batch), actor templates and packed actor keys; rebuilt after
        `to` / `extend` / `select_batch_elements` or when sizes / types tensors are replaced."""
        gen = self.birdview_mesh_generator
        # stamped on the IDENTITY (and version) of the long-lived tensors the cache is derived from -- not on the torch.cat temporaries
        # of get_all_agent_size() / get_all_agent_type(), whose addresses depend on the allocator.  The cache keeps the sources alive.
        sources = [self.agent_size, self.agent_type, gen.background_mesh.verts, gen.background_mesh.faces, gen.background_mesh.attrs]
        if self.npc_count > 0:
            sources += [self.get_npc_size(), self.get_npc_types()]
        for v in (self.traffic_controls or {}).values():
            sources += [v.pos, v.mask]
        extra = (self.batch_size, self.npc_count, tuple((self.traffic_controls or {}).keys()))
        c = self._scene_cache
        if c is not None and c['extra'] == extra and len(c['sources']) == len(sources) and \
                all(a is b and a._version == ver for a, b, ver in zip(sources, c['sources'], c['versions'])):
            return c
        sizes, types = self.get_all_agent_size(), self.get_all_agent_type()
        if not isinstance(self.renderer, HipRenderer):
            raise RuntimeError(f'{type(self.renderer).__name__} cannot take the fused scene path; use HipRenderer')
        dev = sizes.device
        bg = gen.background_mesh                                   # RGBMesh, batch B, (x, y, z) + colour per vertex
        names = list(self.agent_types)
        lv = self.renderer.rendering_levels
        actor_levels = [float(lv[n]) for n in names] + [float(lv['direction']), float(lv['goal_waypoint'])]
        B = self.batch_size
        # traffic controls are drawn like actors without a direction triangle: one quad per stop line (mesh.py:1007-1035)
        controls = self.traffic_controls or {}
        ctrl_kinds = [k for k in controls if controls[k].pos.shape[1] > 0]
        for kind in ctrl_kinds:
            cats = [f'{kind}_{st}' for st in controls[kind].allowed_states] if kind == 'traffic_light' else [kind]
            actor_levels += [float(lv[c]) for c in cats]
        # one device map per DISTINCT mesh of the batch (a collated batch of 512 x Town01 + 512 x Town02 builds two), shared through the
        # process-wide content cache: `copy`, `select_batch_elements`, `extend`, `to` and `shard_simulator` end up here again and find the handles
        smap = self.renderer.scene_maps(bg, actor_levels, device=dev)
        tmpl = actor_template(sizes.detach()).contiguous()          # B x N x 7 x 2 (a render that differentiates the sizes builds its own)
        key_of = lambda name: self._category_key(smap, name)      # noqa: E731
        body = torch.tensor([key_of(n) for n in names], dtype=torch.int64, device=dev)
        dkey = key_of('direction')
        keys = torch.stack([body[types.long()], torch.full_like(types.long(), dkey)], dim=-1).to(torch.int32).contiguous()     # bit pattern of the uint32 key
        key_table = sorted(set(body.tolist()) | {dkey})            # distinct actor keys, known on the host (bit-plane kernel)
        wp_key = key_of('goal_waypoint')
        ctrl = None
        if ctrl_kinds:
            st_q, tm_q, static_keys = [], [], []
            for kind in ctrl_kinds:
                c = controls[kind]
                pos, m = c.pos.to(dev).to(sizes.dtype), c.mask.to(dev)[..., None]
                # padding elements sit at (-1000, -1000) with all four corners there (traffic_controls.py:31-33)
                xy = torch.where(m, pos[..., :2], torch.full_like(pos[..., :2], -1000.0))
                st_q.append(torch.cat([xy, torch.where(m, pos[..., 4:5], torch.zeros_like(pos[..., 4:5])), torch.zeros_like(pos[..., :1])], dim=-1))
                sx = torch.tensor([0.5, -0.5, -0.5, 0.5], dtype=pos.dtype, device=dev) * pos[..., 2:3]      # box2corners_th corner order
                sy = torch.tensor([0.5, 0.5, -0.5, -0.5], dtype=pos.dtype, device=dev) * pos[..., 3:4]
                quad = torch.stack([sx, sy], dim=-1) * m[..., None].to(pos.dtype)
                tm_q.append(torch.cat([quad, torch.zeros(quad.shape[:2] + (3, 2), dtype=pos.dtype, device=dev)], dim=-2))
                if kind == 'traffic_light':
                    static_keys.append(torch.tensor([key_of(f'{kind}_{s_}') for s_ in c.allowed_states], dtype=torch.int64, device=dev))
                else:
                    static_keys.append(torch.full((1,), key_of(kind), dtype=torch.int64, device=dev))
            ctrl = dict(kinds=ctrl_kinds, state=torch.cat(st_q, dim=1).contiguous(), tmpl=torch.cat(tm_q, dim=1).contiguous(), key_lut=static_keys)
            key_table = sorted(set(key_table) | {int(v) for lut in static_keys for v in lut.tolist()})
        self._scene_cache = dict(sources=sources, versions=[t._version for t in sources], extra=extra, map=smap, tmpl=tmpl, keys=keys, key_table=key_table, ctrl=ctrl, wp_key=wp_key)
        return self._scene_cache

    def _category_key(self, smap, name: str) -> int:
        """the key of category `name` in the launches over `smap`: the rank of its rendering level << 24 | its quantised colour
        (ValueError: a level the map does not draw at)"""
        lv, cm = self.renderer.rendering_levels, self.renderer.color_map
        return (smap.rank_of(lv[name]) << 24) | int(_ops.quantise_colors(torch.tensor(cm[name], dtype=torch.float32) / 255.0))

    def _waypoint_triangles(self, waypoints: Tensor, rendering_mask: Optional[Tensor]):
        """B x Nc x M waypoints -> the world-space triangles generate() would add per camera (mesh.py:1120-1145): B x Nc x M*T x 3 x 2.
        The faces of a masked waypoint are zeroed there and so alias the first waypoint vertex of the camera -- a dot at the centre of
        waypoint 0, reproduced here by collapsing the triangle onto that point."""
        disc = self.birdview_mesh_generator.waypoint_mesh
        B, Nc, M = waypoints.shape[:3]
        corner = torch.gather(disc.verts[..., :2].unsqueeze(1).expand(-1, disc.faces.shape[1], -1, -1), 2,
                              disc.faces.long()[..., None].expand(-1, -1, -1, 2))                       # B x T x 3 x 2
        tri = corner[:, None, None].to(waypoints.dtype) + waypoints[..., None, None, :]                     # B x Nc x M x T x 3 x 2
        if rendering_mask is not None:
            first = (disc.verts[:, 0, :2][:, None].to(waypoints.dtype) + waypoints[:, :, 0])[:, :, None, None, None]       # B x Nc x 1 x 1 x 1 x 2
            tri = torch.where(rendering_mask.to(torch.bool)[..., None, None, None], tri, first.expand_as(tri))
        return tri.reshape(B, Nc, M * corner.shape[1], 3, 2).contiguous(), None

    def _control_keys(self, scene) -> Tensor:
        """(B, Nq, 2) int32 keys of the control quads: (colour of the current state, 0 = no direction part)"""
        out = []
        for kind, lut in zip(scene['ctrl']['kinds'], scene['ctrl']['key_lut']):
            c = self.traffic_controls[kind]
            idx = c.state.to(lut.device).long() if kind == 'traffic_light' else torch.zeros_like(c.state.to(lut.device).long())
            out.append(lut[idx])
        body = torch.cat(out, dim=1)
        return torch.stack([body, torch.zeros_like(body)], dim=-1).to(torch.int32)

    def _cameras(self, camera_xy: Tensor, camera_psi: Tensor, camera_sc: Optional[Tensor], rendering_mask: Optional[Tensor]):
        """-> (camera_xy, camera_sc, mask): B x Nc cameras (B x 2 ones become B x 1), their [sin, cos] (`camera_sc`, or of `camera_psi`) and
        the agents each of them sees (present x rendering_mask)"""
        camera_sc = camera_sc if camera_sc is not None else torch.cat([torch.sin(camera_psi), torch.cos(camera_psi)], dim=-1)
        if camera_xy.dim() == 2:
            camera_xy, camera_sc = camera_xy.unsqueeze(1), camera_sc.unsqueeze(1)
        present = self.get_all_agent_present_mask()
        mask = present.unsqueeze(-2).expand(present.shape[:-1] + (camera_xy.shape[-2],) + present.shape[-1:])
        if rendering_mask is not None:
            mask = mask.logical_and(rendering_mask.to(torch.bool))
        return camera_xy, camera_sc, mask

    def _scene_inputs(self, scene, state: Tensor, tmpl: Tensor, mask: Tensor, waypoints: Optional[Tensor], waypoints_rendering_mask: Optional[Tensor]):
        """The agents of a scene launch, from the caller's `state` and templates and the cameras' `mask` -> (state, tmpl, mask, agent_sc, wp_tri):
        the scene's traffic controls appended as quads without a direction triangle, the [sin, cos] of every agent and quad, and the per-camera
        waypoint triangles (None without waypoints)"""
        ctrl = scene['ctrl']
        if ctrl is not None:
            state = torch.cat([state, ctrl['state'].to(state.dtype)], dim=1)
            tmpl = torch.cat([tmpl, ctrl['tmpl'].to(tmpl.dtype)], dim=1)
            mask = torch.cat([mask, torch.ones(mask.shape[:-1] + (ctrl['state'].shape[1],), dtype=torch.bool, device=mask.device)], dim=-1)
        agent_sc = self._heading_sc() if ctrl is None else _ops.heading_sc(state[..., 2])
        wp_tri = None
        if waypoints is not None and waypoints.shape[2] > 0:
            wp_tri, _ = self._waypoint_triangles(waypoints.to(state.dtype), waypoints_rendering_mask)
        return state, tmpl, mask, agent_sc, wp_tri

    def _launch_keys(self, scene, n_cam: int, custom_agent_colors: Optional[Tensor], wp_tri: Optional[Tensor]):
        """-> (keys, key table, per-camera triangles) of a launch: the scene's keys, per camera where `custom_agent_colors` are given (the key
        table is then left to the launch), the control quads' keys appended, and the waypoint key for the triangles `wp_tri`"""
        k, ktab = scene['keys'], scene['key_table']
        if custom_agent_colors is not None:
            # generate() paints the four body vertices of agent a with custom_agent_colors[b, c, a] for camera c
            # (mesh.py:1092-1099); the direction triangle keeps its colour.  Same rendering level, so only the colour
            # bits of the body key change -- per camera.
            rgb = _ops.quantise_colors(custom_agent_colors.to(k.device)).to(torch.int32)          # (B,Nc,A,)
            kc = k[:, None].expand(-1, n_cam, -1, -1).clone()
            kc[..., 0] = (kc[..., 0] & ~0xFFFFFF) | rgb
            k, ktab = kc.contiguous(), None
        if scene['ctrl'] is not None:
            kq = self._control_keys(scene)
            k = torch.cat([k, kq[:, None].expand(-1, n_cam, -1, -1) if k.dim() == 4 else kq], dim=-2).contiguous()
        extra = dict()
        if wp_tri is not None:
            wk = scene['wp_key']
            extra = dict(extra_tri=wp_tri, extra_key=torch.full(wp_tri.shape[:3], wk, dtype=torch.int32, device=wp_tri.device))
            ktab = None if ktab is None else sorted(set(ktab) | {wk})
        return k, ktab, extra

    # ------------------------------------------------------------------------------------------------- rendering
    def _noisy_scene_sources(self):
        """(mesh generator, traffic controls) of a noisy-perception frame (simulator.py:951-978)"""
        from torchdrivesim_amd.mesh import BaseMesh
        from torchdrivesim_amd.utils import rotate
        gen = self.birdview_mesh_generator.copy()
        gen.background_mesh = self.get_noisy_background_mesh()
        noisy_lf = self.get_noisy_lane_features()
        if noisy_lf is not None and noisy_lf.dense_lane_features is not None:
            markers, markers_mask = noisy_lf.dense_lane_features, noisy_lf.dense_lane_features_mask      # B x M x [x, y, psi, width], B x M
            if markers_mask is None:
                markers_mask = torch.ones_like(markers[..., 0], dtype=torch.bool)
            n_markers = markers.shape[-2]
            width = markers[..., 3]
            zero, one = torch.zeros_like(width), torch.ones_like(width)
            arrow = torch.stack([torch.stack([zero, -width / 2], dim=-1), torch.stack([zero, width / 2], dim=-1), torch.stack([one, zero], dim=-1)], dim=-2)
            verts = rotate(arrow, markers[..., None, 2:3]) + markers[..., None, :2]                    # one metre long, pointing along psi
            verts = torch.where(markers_mask[..., None, None], verts, torch.zeros_like(verts))
            faces = torch.tensor([[0, 1, 2]], dtype=torch.long, device=markers.device) + 3 * torch.arange(n_markers, device=markers.device)[:, None]
            dense = BirdviewMesh.set_properties(BaseMesh(verts=verts.flatten(-3, -2), faces=faces.expand_as(verts[..., 0])), category='stop_sign')
            gen.add_static_meshes([dense])
        controls = self.get_noisy_traffic_controls()
        if controls is not None:
            gen.initialize_traffic_controls_mesh(controls)
        return gen, controls

    def render(self, camera_xy: Tensor, camera_psi: Tensor, res: Optional[Resolution] = None, rendering_mask: Optional[Tensor] = None,
               fov: Optional[float] = None, waypoints: Optional[Tensor] = None, waypoints_rendering_mask: Optional[Tensor] = None,
               custom_agent_colors: Optional[Tensor] = None, noisy_perception: bool = False, _camera_sc: Optional[Tensor] = None,
               out: Optional[Tensor] = None, _ego: bool = False) -> Tensor:
        """Bird's-eye images for BxNx2 camera positions and BxNx1 headings -> BxNx3xHxW (simulator.py:920-992).
        `out` (not in the reference, which allocates per call, rendering/cv2.py:52): a caller-owned contiguous BxNx3xHxW tensor of the
        renderer's output dtype to render into; returned.  HipRenderer only, one static map per batch, not for differentiable calls."""
        if noisy_perception:
            # what the policy is shown instead of the truth (simulator.py:951-978): the observation model's background, its lane markers
            # drawn as triangles, its traffic controls.  The scene of the ordinary path is swapped for the duration of the call; its
            # static map is rebuilt from the noisy background (a map upload per call: this is the slow lane of the renderer).
            gen, controls = self._noisy_scene_sources()
            saved = (self.birdview_mesh_generator, self.traffic_controls, self._scene_cache)
            self.birdview_mesh_generator, self.traffic_controls, self._scene_cache = gen, controls, None
            try:
                return self.render(camera_xy, camera_psi, res=res, rendering_mask=rendering_mask, fov=fov, waypoints=waypoints,
                                   waypoints_rendering_mask=waypoints_rendering_mask, custom_agent_colors=custom_agent_colors,
                                   noisy_perception=False, _camera_sc=_camera_sc, out=out, _ego=_ego)
            finally:
                self.birdview_mesh_generator, self.traffic_controls, self._scene_cache = saved
        camera_xy, camera_sc, mask = self._cameras(camera_xy, camera_psi, _camera_sc, rendering_mask)
        n_cam = camera_xy.shape[-2]
        if isinstance(self.renderer, HipRenderer):
            scene = self._scene()
            state = self.get_all_agent_state()
            # gradients through the rasteriser (K3 backward, build-defined) only when someone asks for them
            sizes = self.get_all_agent_size()
            size_grad = torch.is_grad_enabled() and sizes.requires_grad and self.renderer.out_dtype == torch.float32
            diff = torch.is_grad_enabled() and (state.requires_grad or camera_xy.requires_grad or camera_sc.requires_grad or size_grad) and \
                self.renderer.out_dtype == torch.float32
            if not diff:
                state, camera_xy, camera_sc = state.detach(), camera_xy.detach(), camera_sc.detach()
            # gradients with respect to the agents' length and width flow through the template vertices (actor_template is plain torch)
            tmpl_all = actor_template(sizes).contiguous() if size_grad else scene['tmpl']
            state, tmpl_all, mask, agent_sc, wp_tri = self._scene_inputs(scene, state, tmpl_all, mask, waypoints, waypoints_rendering_mask)
            # the metrics run beside the launch; a differentiable render forks too when the launch stays on the caller's stream (the plain second
            # stream, or 'reserved' with the loop on sim.raster_stream()): the metric nodes are then autograd nodes of the side stream, and the
            # engine runs their backward there as well -- beside the rasteriser's backward
            if not diff or self.overlap_infractions is True or \
                    (self.overlap_infractions == 'reserved' and state.is_cuda and self._reserved_usable(state.device) and
                     torch.cuda.current_stream(state.device) == _ops.reserved_streams(state.device, Simulator._reserved_per_xcd)[0]):
                r = res if res is not None else getattr(self.renderer, 'res', None)
                self._mark_fork(write_bound=self.renderer.out_dtype == torch.float32 and (r is None or min(r.height, r.width) > 208))
            # render_egocentric with gradients: the cameras are the exposed agents themselves -- one autograd node takes state and headings and
            # folds the cameras' gradient into the agents' (no slice nodes for camera_xy / camera_sc in the graph)
            ego_n = n_cam if (_ego and diff and scene['ctrl'] is None and n_cam <= state.shape[1]) else 0
            k, ktab, extra = self._launch_keys(scene, n_cam, custom_agent_colors, wp_tri)
            # 'reserved' and a plain launch that goes to the stream kept off the reserved CUs (the loop's own stream, or the detour below): the
            # metric stream -- the foreseen metrics are on it by now -- is the launch's helper stream (`_ops.use_helper_cus`)
            helper = None
            if self.overlap_infractions == 'reserved' and not diff and state.is_cuda and self._reserved_usable(state.device):
                rs0, ms0 = _ops.reserved_streams(state.device, Simulator._reserved_per_xcd)
                if torch.cuda.current_stream(state.device) == rs0 or (self._fork is not None and self._fork[2] != rs0):
                    helper = ms0
            launch = lambda: self.renderer.render_scene(scene['map'], state, agent_sc, tmpl_all, k, mask.contiguous(), camera_xy, camera_sc,     # noqa: E731
                                                        res=res, fov=fov, key_table=ktab, differentiable=diff, **extra, out=out, ego_cameras=ego_n,
                                                        helper_stream=helper)
            if self.overlap_infractions == 'reserved' and not diff and self._fork is not None and state.is_cuda and \
                    self._fork[2] != _ops.reserved_streams(state.device, Simulator._reserved_per_xcd)[0]:
                # the launch goes to the stream that is kept off the reserved CUs: it waits for what the caller's stream has enqueued so far
                # (the fork event) and the caller's stream waits for it -- beside it, on the reserved CUs, the foreseen metrics are running.
                # (A loop that makes that stream its current one -- `with torch.cuda.stream(sim.raster_stream()):` -- saves these two waits.)
                main = self._fork[2]
                rs = _ops.reserved_streams(state.device, Simulator._reserved_per_xcd)[0]
                # NOT the fork event: the per-launch inputs (per-camera colour keys, traffic-control keys, waypoint triangles and their
                # keys) were built on the caller's stream AFTER it -- the launch waits for an event recorded here, behind all of them
                built = torch.cuda.Event()
                built.record(main)
                rs.wait_event(built)
                with torch.cuda.stream(rs):
                    img = launch()
                img.record_stream(main)
                done = torch.cuda.Event()
                done.record(rs)
                main.wait_event(done)
                return img
            return launch()
        if out is not None:
            raise RuntimeError(f'`out=` is served by HipRenderer only, not by {type(self.renderer).__name__}')
        # any other BirdviewRenderer: the reference's generic dataflow (explicit per-camera mesh)
        rgb_mesh = self.birdview_mesh_generator.generate(n_cam, agent_state=self.get_all_agent_state()[:, None].expand(-1, n_cam, -1, -1),
                                                         present_mask=mask, custom_agent_colors=custom_agent_colors,
                                                         waypoints=waypoints, waypoints_rendering_mask=waypoints_rendering_mask,
                                                         traffic_lights=self.traffic_controls['traffic_light'].extend(n_cam, in_place=False)
                                                         if self.traffic_controls and 'traffic_light' in self.traffic_controls else None)
        img = self.renderer.render_frame(rgb_mesh, camera_xy, camera_sc, res=res, fov=fov)
        return img.reshape((self.batch_size, n_cam) + img.shape[1:])

    def render_egocentric(self, ego_rotate: bool = True, res: Optional[Resolution] = None, fov: Optional[float] = None,
                          visibility_matrix: Optional[Tensor] = None, custom_agent_colors: Optional[Tensor] = None,
                          n_subsequent_waypoints: int = 1, noisy_perception: bool = False, out: Optional[Tensor] = None) -> Tensor:
        """One camera per exposed agent -> BxAx3xHxW (simulator.py:994-1033).  `out`: see `render`."""
        return self.render(**self._egocentric_cameras(ego_rotate, visibility_matrix, n_subsequent_waypoints), res=res, fov=fov,
                           custom_agent_colors=custom_agent_colors, noisy_perception=noisy_perception, out=out, _ego=ego_rotate)

    def _egocentric_cameras(self, ego_rotate: bool, visibility_matrix: Optional[Tensor], n_subsequent_waypoints: int):
        """the cameras of `render_egocentric`, one per exposed agent, as keyword arguments of `render` / `render_semantic`"""
        state = self.get_state()
        camera_xy, camera_psi = state[..., :2], state[..., 2:3]
        if not ego_rotate:
            camera_psi = torch.ones_like(camera_psi) * (np.pi / 2)
        rendering_mask = visibility_matrix
        if self.cfg.single_agent_rendering:
            # the reference builds eye(2) here regardless of A; the intended eye(A) over all agents is used
            A, total = self.agent_count, self.agent_count + self.npc_count
            rendering_mask = torch.eye(A, total, dtype=torch.bool, device=state.device).unsqueeze(0).expand(self.batch_size, -1, -1)
        cam_sc = None
        if ego_rotate:
            cam_sc = self._heading_sc()                                     # the cameras ARE the exposed agents (differentiable when the state is)
            if cam_sc.shape[-2] != self.agent_count:
                cam_sc = cam_sc[..., :self.agent_count, :]
        waypoints = self.get_waypoints(count=n_subsequent_waypoints)                  # simulator.py:1013-1017
        waypoints_mask = self.get_waypoints_mask(count=n_subsequent_waypoints) if waypoints is not None else None
        return dict(camera_xy=camera_xy, camera_psi=camera_psi, rendering_mask=rendering_mask, waypoints=waypoints,
                    waypoints_rendering_mask=waypoints_mask, _camera_sc=cam_sc)

    # ------------------------------------------------------------------------------------------------- semantic masks
    def _category_keys(self, scene) -> Dict[str, int]:
        """category -> its key in this scene's launches (rank of its rendering level << 24 | its colour, as _scene() builds them), for every
        category with a level and a colour whose level the map's level table holds"""
        out = {}
        for n in self.renderer.rendering_levels:
            if n not in self.renderer.color_map:
                continue
            try:
                out[n] = self._category_key(scene['map'], n)
            except ValueError:                                       # a level this scene never draws at
                continue
        return out

    def semantic_channels(self) -> List[str]:
        """The default channels of `render_semantic`: one per category that has a key in this scene (map faces, agent types and their
        direction triangle, traffic controls, waypoint goals), from the lowest-priority rendering level (road) to the highest (direction),
        ties broken by name."""
        if not isinstance(self.renderer, HipRenderer):
            raise NotImplementedError(f'semantic masks are rendered by HipRenderer only, not by {type(self.renderer).__name__}')
        scene = self._scene()
        present = set(scene['map'].face_keys() or ()) | set(scene['key_table'])
        if self.waypoint_goals is not None:
            present.add(scene['wp_key'])
        lv = self.renderer.rendering_levels
        return sorted((n for n, k in self._category_keys(scene).items() if k in present), key=lambda n: (-float(lv[n]), n))

    def _semantic_spec(self, scene, channels):
        """channels (names or collections of names) -> (the channels as tuples, key -> channel set)"""
        chans = [(c,) if isinstance(c, str) else tuple(c) for c in (self.semantic_channels() if channels is None else channels)]
        if not 1 <= len(chans) <= 32:
            raise ValueError(f'semantic masks take 1 to 32 channels, got {len(chans)}')
        lv, cm = self.renderer.rendering_levels, self.renderer.color_map
        keys = self._category_keys(scene)
        key_channels = {}
        for i, cats in enumerate(chans):
            for name in cats:
                if name not in lv or name not in cm:
                    raise ValueError(f'unknown category {name!r} in channel {i} (categories: {sorted(n for n in lv if n in cm)})')
            for name in cats:
                k = keys.get(name)
                if k is None:
                    continue                                         # valid, but never drawn with this map: an all-zero contribution
                for other, ko in keys.items():
                    if ko == k and other not in cats:
                        raise ValueError(f'channel {i} names {name!r}, which shares its key (colour and rendering level) with {other!r}, '
                                         f'which the channel does not name')
                key_channels[k] = key_channels.get(k, 0) | (1 << i)
        return chans, key_channels

    def render_semantic(self, camera_xy: Tensor, camera_psi: Tensor, channels=None, res: Optional[Resolution] = None, fov: Optional[float] = None,
                        rendering_mask: Optional[Tensor] = None, waypoints: Optional[Tensor] = None, waypoints_rendering_mask: Optional[Tensor] = None,
                        packed: bool = False, out: Optional[Tensor] = None, _camera_sc: Optional[Tensor] = None) -> Tensor:
        """Semantic bird's-eye masks for the cameras of `render` -> BxNcxCxHxW bool (packed: BxNcxCxceil(W/32)xH int32 words,
        `rendering.unpack_mask_bits`).  `channels`: a list of C <= 32 entries, each a category name or a collection of names (their union);
        default `semantic_channels()`.  Channel c is set at a pixel exactly where `render` would paint a face of one of its categories -- the
        same faces, masks, stop lines, light states and waypoint discs -- whatever is drawn over it (a road channel stays set under a car).
        Categories map to keys through the renderer's colour map and rendering levels; agents take the colour of their type.  A category that
        this scene never draws gives an all-zero channel; an unknown name, or a category that shares its colour and level with one the channel
        does not name, is a ValueError.  A plain launch on the current stream, never differentiable; `out`: a caller-owned tensor of the result's
        shape and dtype.  HipRenderer only."""
        if not isinstance(self.renderer, HipRenderer):
            raise NotImplementedError(f'semantic masks are rendered by HipRenderer only, not by {type(self.renderer).__name__}')
        scene = self._scene()
        chans, key_channels = self._semantic_spec(scene, channels)
        camera_xy, camera_sc, mask = self._cameras(camera_xy, camera_psi, _camera_sc, rendering_mask)
        state, tmpl, mask, agent_sc, wp_tri = self._scene_inputs(scene, self.get_all_agent_state().detach(), scene['tmpl'], mask, waypoints,
                                                                 waypoints_rendering_mask)
        keys, ktab, extra = self._launch_keys(scene, camera_xy.shape[-2], None, wp_tri)
        return self.renderer.render_scene_masks(scene['map'], state, agent_sc, tmpl, keys, mask.contiguous(), camera_xy, camera_sc, key_channels,
                                                len(chans), res=res, fov=fov, key_table=ktab, packed=packed, out=out, **extra)

    def render_egocentric_semantic(self, ego_rotate: bool = True, channels=None, res: Optional[Resolution] = None, fov: Optional[float] = None,
                                   visibility_matrix: Optional[Tensor] = None, n_subsequent_waypoints: int = 1, packed: bool = False,
                                   out: Optional[Tensor] = None) -> Tensor:
        """`render_semantic` with one camera per exposed agent, the cameras, masks and waypoint goals of `render_egocentric` -> BxAxCxHxW."""
        return self.render_semantic(**self._egocentric_cameras(ego_rotate, visibility_matrix, n_subsequent_waypoints), channels=channels, res=res,
                                    fov=fov, packed=packed, out=out)

    # ------------------------------------------------------------------------------------------------- infractions
    def compute_offroad(self) -> Tensor:
        """BxA off-road loss = thresholded squared corner-to-mesh distance x present (simulator.py:1035-1044).
        The whole road_mesh is the driving surface, lane markings included."""
        return self._beside_render(self._compute_offroad, ('offroad',))

    def _compute_offroad(self) -> Tensor:
        state = self.get_state()
        if self.agent_count == 0 or self.road_mesh.faces_count == 0:
            return torch.zeros_like(state[..., 0])
        from torchdrivesim_amd.infractions import _static_maps_for
        smap = _static_maps_for(self.road_mesh, state.device)      # geometry-only device map, cached on the mesh
        size, present = self.get_agent_size(), self.get_present_mask()
        sc = self._heading_sc()
        if sc.shape[-2] != self.agent_count:
            sc = sc[..., :self.agent_count, :]
        return _ops.offroad(smap, state, size, threshold=self.cfg.offroad_threshold, present=present, sc=sc)

    # ------------------------------------------------------------------------------------------------- range scans
    @staticmethod
    def range_scan_angles(n_rays: int, fov: float = 2 * np.pi, device=None) -> Tensor:
        """(R,) float32 offsets of the rays from the agent's heading, counter-clockwise: off_k = -fov/2 + fov * (k + 0.5) / R, evaluated in
        float64 on `device` (default: the host) and rounded once.  The division is by a TENSOR: torch divides by a host scalar through its
        reciprocal on the GPU, and the offsets are the same bits wherever they are computed."""
        _ops.check_range_scan_args(n_rays, 0.0, 0.0)
        if not (np.isfinite(fov) and fov > 0):
            raise ValueError(f'range scan: fov must be finite and positive (got {fov})')
        k = torch.arange(int(n_rays), dtype=torch.float64, device=device)
        return (-fov / 2 + (fov * (k + 0.5)) / torch.full((), int(n_rays), dtype=torch.float64, device=device)).to(torch.float32)

    def compute_range_scan(self, n_rays: int = 64, max_range: float = 50.0, fov: float = 2 * np.pi, gap_tolerance: float = 0.02, road: bool = True,
                           agents: bool = True, differentiable: bool = False) -> RangeScan:
        """A lidar-like observation of every exposed agent: `n_rays` rays from the agent's centre, ray k at the angle psi + off_k
        (`range_scan_angles`; counter-clockwise in world coordinates, as psi), each reporting in metres

        agents  BxAxR  the smallest t >= 0 at which the ray enters the oriented rectangle of any OTHER present entity (exposed agents and NPCs;
                       0 from inside one), `max_range` without one below `max_range`;
        road    BxAxR  the length of the ray's initial stretch that lies on `road_mesh` (the whole of it, lane markings included, as in
                       `compute_offroad`): with [a_f, b_f] the stretch of the ray inside the closed face f -- faces of positive area only --
                       the least fixed point of F <- max{b_f : a_f <= F + gap_tolerance} from F = 0, capped at `max_range`; 0 for an agent whose
                       centre is off the road.  `gap_tolerance` bridges the hairline gaps between separately triangulated lanelets;
        hit     BxAxR  int32: the index in [0, A + Npc) of the entity that defines `agents` where agents < max_range and agents <= road (the
                       lowest index on a tie), -2 where road < max_range and road < agents, -1 where both are `max_range`.

        Without a road mesh or with road=False every `road` is `max_range`; with agents=False every `agents` is.  Rows of exposed agents that are not
        present hold max_range, max_range, -1.  [sin, cos] of the rays come from torch.sin / torch.cos on the device; the rest is one HIP kernel in
        binary32 (csrc/scan.hip; parity: tests/range_scan_model.py, a float64 model).  Runs on the current stream, allocates its
        outputs only, and reuses the cached off-road map: once that map exists (one eager call, or `compute_offroad`, on this road mesh) the call
        can be captured into a graph -- nothing crosses from the host, the ray offsets are built on the device.

        `differentiable=True`, with grad mode on and a state or size that requires grad: the same launch and the same bits, and `agents` and
        `road` carry the graph to x, y and psi of the observing agent (psi through the rays' [sin, cos] and the shared [sin psi, cos psi] node)
        and to x, y, psi and the size of the entity a ray ends on; `hit` never does.  The backward is one HIP kernel (csrc/scan_bwd.hip;
        include/tdship.h "K5b", held to the float64 model tests/range_scan_grad_model.py).  Constants of differentiation: the entity and the
        side of its rectangle that define `agents`, the road edge `road` ends on, the map, `max_range`, `gap_tolerance` and `fov`.  A ray that is
        capped at `max_range`, starts inside a rectangle or off the road, or belongs to an absent agent contributes exactly zero whatever
        gradient comes in, NaN and inf included.  Otherwise -- the flag off, under `no_grad`, nothing requiring grad -- nothing is recorded
        and nothing is saved."""
        _ops.check_range_scan_args(n_rays, max_range, gap_tolerance)
        if not (np.isfinite(fov) and fov > 0):
            raise ValueError(f'range scan: fov must be finite and positive (got {fov})')
        state = self.get_state()
        if not state.is_cuda:
            raise RuntimeError(f'compute_range_scan runs on an MI355X; the simulator is on {state.device} (no CPU fallback)')
        B, A, R = state.shape[0], self.agent_count, int(n_rays)
        if A == 0:
            empty = torch.empty((B, 0, R), dtype=torch.float32, device=state.device)
            return RangeScan(empty, empty.clone(), torch.empty((B, 0, R), dtype=torch.int32, device=state.device))
        smap = None
        if road and self.road_mesh.faces_count > 0:
            from torchdrivesim_amd.infractions import _static_maps_for
            smap = _static_maps_for(self.road_mesh, state.device)      # the geometry-only device map of compute_offroad, cached on the mesh
        if differentiable and torch.is_grad_enabled():
            all_state, size = self.get_all_agent_state(), self.get_all_agent_size()
            if all_state.requires_grad or size.requires_grad:
                boxes = _ops.state_boxes(all_state, size)
                ray_sc = _ops.heading_sc(state[..., 2].unsqueeze(-1) + self.range_scan_angles(R, fov, device=state.device))
                return RangeScan(*_ops.range_scan_grad(smap, boxes, self._heading_sc(), self.get_all_agent_present_mask(), ray_sc, A, max_range,
                                                       gap_tolerance, want_agents=agents))
        with torch.no_grad():
            all_state = self.get_all_agent_state().detach()
            boxes = torch.cat([all_state[..., :2], self.get_all_agent_size().detach(), all_state[..., 2:3]], dim=-1)
            sc = self._heading_sc().detach()
            ray_sc = _ops.heading_sc(state[..., 2].detach().unsqueeze(-1) + self.range_scan_angles(R, fov, device=state.device))
            out = _ops.range_scan(smap, boxes, sc, self.get_all_agent_present_mask(), ray_sc, A, max_range, gap_tolerance, want_agents=agents)
        return RangeScan(*out)

    # ------------------------------------------------------------------------------------------------- neighbour observations
    def _entities_no_grad(self):
        """all entities as K6 and K9 read them, off the graph -> boxes Bx(A+Npc)x5 [x, y, length, width, psi], [sin, cos] of psi, speed, present"""
        with torch.no_grad():
            all_state = self.get_all_agent_state().detach()
            boxes = torch.cat([all_state[..., :2], self.get_all_agent_size().detach(), all_state[..., 2:3]], dim=-1)
            return boxes, self._heading_sc().detach(), all_state[..., 3], self.get_all_agent_present_mask()

    def compute_neighbors(self, k: int = 8, max_distance: float = 50.0, visible: Optional[Tensor] = None, differentiable: bool = False) -> Neighbors:
        """The `k` nearest OTHER present entities (exposed agents and NPCs) of every exposed agent within `max_distance` metres between centres
        (+inf: no limit), nearest first, equal distances by the lower entity index:

        features  BxAxkx8  per slot `Neighbors.FEATURES`: x, y of the neighbour's centre in the observer's frame (x ahead, y to the left), [sin, cos]
                           of its heading relative to the observer's, vx, vy its velocity minus the observer's in the observer's frame, its length
                           and width; all 0 in an empty slot;
        index     BxAxk    int32: the entity in [0, A + Npc) of the slot, -1 for an empty slot (`Neighbors.mask`; `Neighbors.take` gathers any
                           per-entity tensor at it).

        `visible`: an optional BxAx(A+Npc) bool or uint8 tensor, non-zero where observer a may see entity e -- `get_noisy_present_mask()` of an
        occlusion noise model is one.  Rows of exposed agents that are not present are empty.  1 <= k <= 32, at most 1024 entities per scene.
        One HIP kernel in binary32 (csrc/neighbors.hip; the definition is in include/tdship.h, tests/neighbors_model.py equals it bit for bit).
        Runs on the current stream and allocates its outputs only, so it can be captured into a graph.

        `differentiable=True`, with grad mode on and a state or size that requires grad: the same launch and the same bits, and `features`
        carries the graph to x, y, psi (through the shared [sin psi, cos psi] node) and the speed of both entities of every filled slot and to
        the size of the slot's entity; `index` never does.  The backward is one HIP kernel (csrc/neighbors_bwd.hip; include/tdship.h "K6b",
        held to the float64 model tests/neighbors_grad_model.py).  Constants of differentiation: which entity is in a slot and the
        `max_distance` cut, `visible`, the order of the slots.  An empty slot contributes exactly zero whatever gradient comes in, NaN and
        inf included; a filled slot whose inputs are not finite propagates what IEEE arithmetic gives.  Otherwise -- the flag off, under
        `no_grad`, nothing requiring grad -- nothing is recorded and nothing is saved."""
        _ops.check_neighbors_args(k, max_distance)
        state = self.get_state()
        if not state.is_cuda:
            raise RuntimeError(f'compute_neighbors runs on an MI355X; the simulator is on {state.device} (no CPU fallback)')
        B, A, K = state.shape[0], self.agent_count, int(k)
        if A == 0:
            return Neighbors(torch.empty((B, 0, K, 8), dtype=torch.float32, device=state.device), torch.empty((B, 0, K), dtype=torch.int32, device=state.device))
        if differentiable and torch.is_grad_enabled():
            all_state, size = self.get_all_agent_state(), self.get_all_agent_size()
            if all_state.requires_grad or size.requires_grad:
                boxes = _ops.state_boxes(all_state, size)
                return Neighbors(*_ops.neighbors_grad(boxes, self._heading_sc(), all_state[..., 3], self.get_all_agent_present_mask(), A, K, max_distance,
                                                      visible))
        return Neighbors(*_ops.neighbors(*self._entities_no_grad(), A, K, max_distance, visible=visible))

    # ------------------------------------------------------------------------------------------------- time to collision
    def compute_time_to_collision(self, k: int = 1, horizon: float = 5.0, margin: float = 0.0, visible: Optional[Tensor] = None,
                                  differentiable: bool = False) -> TimeToCollision:
        """When every exposed agent would first touch another present entity (exposed agents and NPCs) if everybody kept its current velocity
        `v * [cos psi, sin psi]` and heading: the `k` soonest within `horizon` seconds (+inf: no limit), equal times by the lower entity index:

        ttc    BxAxk  float32 seconds, 0 for a pair whose rectangles overlap already, +inf in an empty slot (`TimeToCollision.min` is slot 0);
        index  BxAxk  int32: the entity in [0, A + Npc) of the slot, -1 for an empty slot (`TimeToCollision.mask`, `TimeToCollision.take`).

        `margin` metres are added to the observing agent's rectangle on every side.  `visible` is that of `compute_neighbors`.  Rows of exposed
        agents that are not present, or whose pose, size or speed is not finite, are empty.  1 <= k <= 32, at most 1024 entities per scene.
        One HIP kernel in binary64 (csrc/ttc.hip; the definition is in include/tdship.h "K9", tests/ttc_model.py equals it bit for bit).
        Runs on the current stream and allocates its outputs only, so it can be captured into a graph.

        `differentiable=True`, with grad mode on and a state or size that requires grad: the same launch and the same bits, and `ttc` carries the
        graph to x, y, psi (through the shared [sin psi, cos psi] node), the speed and the sizes of both entities of every slot; `index` never
        does.  The backward is one HIP kernel (csrc/ttc_bwd.hip; include/tdship.h "K9b", held to the float64 model tests/ttc_grad_model.py).
        Constants of differentiation: which entity is in a slot, the separating axis that binds, the sign of the closing speed on it and the
        signs inside the projected extents; `margin` and `horizon` get no gradient.  A slot contributes iff it is filled and its time is above
        0: an empty slot (+inf) and a pair that overlaps already (0) contribute exactly zero whatever gradient comes in.  Otherwise -- the flag
        off, under `no_grad`, nothing requiring grad -- nothing is recorded and nothing is saved."""
        _ops.check_ttc_args(k, horizon, margin)
        state = self.get_state()
        if not state.is_cuda:
            raise RuntimeError(f'compute_time_to_collision runs on an MI355X; the simulator is on {state.device} (no CPU fallback)')
        B, A, K = state.shape[0], self.agent_count, int(k)
        if A == 0:
            return TimeToCollision(torch.empty((B, 0, K), dtype=torch.float32, device=state.device), torch.empty((B, 0, K), dtype=torch.int32, device=state.device))
        if differentiable and torch.is_grad_enabled():
            all_state, size = self.get_all_agent_state(), self.get_all_agent_size()
            if all_state.requires_grad or size.requires_grad:
                boxes = _ops.state_boxes(all_state, size)
                return TimeToCollision(*_ops.time_to_collision_grad(boxes, self._heading_sc(), all_state[..., 3], self.get_all_agent_present_mask(), A, K,
                                                                    horizon, margin, visible))
        return TimeToCollision(*_ops.time_to_collision(*self._entities_no_grad(), A, K, horizon, margin, visible=visible))

    # ------------------------------------------------------------------------------------------------- stop-line observations
    def compute_stop_lines(self, k: int = 4, max_distance: float = 60.0, ahead_only: bool = True, min_cos: Optional[float] = None,
                           kind: str = 'traffic_light', differentiable: bool = False) -> StopLines:
        """The `k` nearest present stop lines of `traffic_controls[kind]` of every exposed agent within `max_distance` metres between centres
        (+inf: no limit), nearest first, equal distances by the lower index:

        features  BxAxkx8  per slot `StopLines.FEATURES`: x, y of the line's centre in the agent's frame (x ahead, y to the left), [sin, cos] of the
                           line's orientation relative to the agent's heading, its length and width, the seconds until its light changes (0 for a
                           control without a programme) and the distance; all 0 in an empty slot;
        index     BxAxk    int32: the stop line of the slot, -1 for an empty slot (`StopLines.mask`; `StopLines.take` gathers at it);
        state     BxAxk    int32: the line's index into the control's `allowed_states`, -1 for an empty slot.

        `ahead_only` keeps the lines with x >= 0; `min_cos` those whose relative orientation has at least that cosine.  Rows of agents that are not
        present are empty.  1 <= k <= 32, at most 1024 lines per scene.  One HIP kernel in binary32 (csrc/lights.hip; the definition is in
        include/tdship.h "K7", tests/lights_model.py equals it bit for bit).  Runs on the current stream and allocates its outputs only, so it
        can be captured into a graph.

        `differentiable=True`, with grad mode on and a state that requires grad: the same launch and the same bits, and `features` carries the
        graph to x, y and psi (through the shared [sin psi, cos psi] node) of the observing agent -- the stop lines are constants, even where
        `control.pos` requires grad, so nothing goes to them or to another entity; `index` and `state` never carry a graph.  The backward is one
        HIP kernel (csrc/stop_lines_bwd.hip; include/tdship.h "K7b", held to the float64 model tests/stop_lines_grad_model.py).  Constants of
        differentiation: which line is in a slot and the order of the slots, the `max_distance` cut, `ahead_only`, `min_cos` and the control's
        mask; `time_to_change`, length and width receive gradient from nowhere and send none.  An empty slot contributes exactly zero whatever
        gradient comes in, NaN and inf included; an agent exactly on a line's centre gets no NaN from `distance`.  Otherwise -- the flag off,
        under `no_grad`, nothing requiring grad, no agents -- nothing is recorded and nothing is saved."""
        _ops.check_stop_lines_args(k, max_distance, min_cos)
        controls = self.get_traffic_controls()
        if not controls or kind not in controls:
            raise ValueError(f'compute_stop_lines: the simulator has no {kind!r} traffic controls')
        control = controls[kind]
        state = self.get_state()
        if not state.is_cuda:
            raise RuntimeError(f'compute_stop_lines runs on an MI355X; the simulator is on {state.device} (no CPU fallback)')
        A = self.agent_count
        with torch.no_grad():
            pos = control.pos
            key = (pos.data_ptr(), pos._version, tuple(pos.shape), str(pos.device))
            cached = getattr(control, '_line_sc_cache', None)
            if cached is None or cached[0] != key:                      # the stop lines do not move: their [sin, cos] is computed once
                lines = _ops._c(pos.detach()).to(state.device)
                cached = (key, lines, _ops.heading_sc(lines[..., 4]))
                control._line_sc_cache = cached
        if differentiable and A > 0 and torch.is_grad_enabled() and state.requires_grad:
            return StopLines(*_ops.stop_lines_grad(state[..., :2], self._heading_sc()[:, :A], self.get_present_mask(), cached[1], cached[2], control.mask,
                                                   control.state, getattr(control, 'time_to_change', None), k, max_distance, ahead_only=ahead_only,
                                                   min_cos=min_cos))
        with torch.no_grad():
            agent = state.detach()
            out = _ops.stop_lines(agent[..., :2], self._heading_sc().detach()[:, :A], self.get_present_mask(), cached[1], cached[2], control.mask,
                                  control.state, getattr(control, 'time_to_change', None), k, max_distance, ahead_only=ahead_only, min_cos=min_cos)
        return StopLines(*out)

    # ------------------------------------------------------------------------------------------------- lane observations
    def compute_lanes(self, k: int = 6, n_points: int = 8, spacing: float = 4.0, max_distance: float = 30.0, differentiable: bool = False) -> Lanes:
        """The `k` nearest lanelets of `lanelet_map` of every exposed agent, by the distance to their centre lines, within `max_distance` metres
        (+inf: no limit), nearest first, equal float32 distances by the lower lanelet index.  The lanelets are those `snap_to_lanes` looks at:
        long enough to drive on and without an excluded tag.

        features  BxAxkx8    per slot `Lanes.FEATURES`: x, y of the foot -- the closest point of the centre line -- in the agent's frame (x ahead, y
                             to the left), [sin, cos] of the lane's direction there relative to the agent's heading (an oncoming lane has cos < 0),
                             the foot's arc length on the lanelet, the length that remains after it, the agent's lateral offset from the line
                             (left positive, as `snap_to_lanes`) and the distance; all 0 in an empty slot;
        points    BxAxkxPx2  the centre line ahead of the foot in the agent's frame, point j `j * spacing` metres after it; the line goes on into
                             the next lanelet while there is exactly one successor (at most 8 times) and ends at a fork or a dead end -- the
                             branches are slots of their own where they are in range;
        n_valid   BxAxk      int32: the points of the slot that are on the lane (`Lanes.points_mask`), the others are 0; at least 1 in a filled slot;
        index     BxAxk      int32: the lanelet of the slot in its scene's `laneletLayer`, -1 for an empty slot (`Lanes.mask`).

        Rows of agents that are not present, whose pose is NaN, or whose scene has no lanelet map (an entry `None`) are empty; without any lanelet
        map everything is empty and nothing is launched.  1 <= k <= 32, 1 <= n_points <= 32, at most 2048 lanelets per map.  One HIP kernel in
        binary64 (csrc/lane_obs.hip; the definition is in include/tdship.h "K8", tests/lane_obs_model.py equals it bit for bit).
        Runs on the current stream and allocates its outputs only; the device lane tables are those of `compute_wrong_way`, built by the first
        call of either -- which must happen outside a stream capture; after that the call can be captured into a graph.

        `differentiable=True`, with grad mode on and a state that requires grad: the same launch and the same bits, and `features` and `points`
        carry the graph to x, y and psi (through the shared [sin psi, cos psi] node) of the observing agent -- the map is constant, so nothing
        goes to another entity; `n_valid` and `index` never do.  The backward is one HIP kernel (csrc/lane_obs_bwd.hip; include/tdship.h "K8b",
        held to the float64 model tests/lane_obs_grad_model.py).  Constants of differentiation: which lanelet is in a slot and the order of the
        slots, the `max_distance` cut, the segment the foot lies on, whether the foot was clamped to a segment's end, and for every point
        whether it is valid and the lanelet and segment it lies on.  Where the foot is not clamped the polyline slides along the lane as the
        agent moves, and the gradient of the points says so.  An empty slot and an invalid point contribute exactly zero whatever gradient
        comes in, NaN and inf included; an agent exactly on a centre line gets no NaN from `distance`.  Otherwise -- the flag off, under
        `no_grad`, nothing requiring grad, no lanelet map, no agents -- nothing is recorded and nothing is saved."""
        _ops.check_lanes_args(k, n_points, spacing, max_distance)
        state = self.get_state()
        if not state.is_cuda:
            raise RuntimeError(f'compute_lanes runs on an MI355X; the simulator is on {state.device} (no CPU fallback)')
        B, A = state.shape[0], self.agent_count
        if A == 0 or self.lanelet_map is None or all(m is None for m in self.lanelet_map):
            return Lanes(*_ops.empty_lane_observations(B, A, int(k), int(n_points), state.device))
        if differentiable and torch.is_grad_enabled() and state.requires_grad:
            return Lanes(*_ops.lane_observations_grad(self._lane_tables(state.device), state[..., :2], self._heading_sc()[:, :A], self.get_present_mask(),
                                                      k, n_points, spacing, max_distance))
        with torch.no_grad():
            agent = state.detach()
            out = _ops.lane_observations(self._lane_tables(state.device), agent[..., :2], self._heading_sc().detach()[:, :A], self.get_present_mask(),
                                         k, n_points, spacing, max_distance)
        return Lanes(*out)

    def _lane_tables(self, device) -> _ops.LaneTableSet:
        """the device lane tables of `lanelet_map`, made on the first call and kept (allocations and copies: outside any stream capture)"""
        tol = self.cfg.lanelet_inclusion_tolerance
        if self._lane_set is None or self._lane_set[1] < tol or self._lane_set[0].device != device:
            self._lane_set = (lane_table_set(self.lanelet_map, device, tol), tol)
        return self._lane_set[0]

    def compute_wrong_way(self, differentiable: bool = False) -> Tensor:
        """Wrong-way metric per agent, -cos of the angle between the agent and the lane it is on where that angle exceeds
        `cfg.wrong_way_angle_threshold` (simulator.py:607-630 -> infractions.lanelet_orientation_loss), times the present mask.
        Zeros without a lanelet map, as the reference.  `lanelet_map`: a list of B `lanelet2.LaneletMap` or None.

        `differentiable=True`, with grad mode on and a state that requires grad: the same bits, and the result carries the graph to psi alone,
        as the reference's loss does (`_ops.wrong_way_grad`): -sin of that angle for the lanelet that attains the minimum
        where the angle exceeds the threshold, else 0; x and y get exactly zero.  This call is computed in place on the current stream: it is
        not foreseen beside a render, and a result prepared there is not used.  Otherwise -- the flag off, under `no_grad`, nothing requiring
        grad, no lanelet map -- the path is the plain one and nothing is recorded."""
        if differentiable and torch.is_grad_enabled() and self.get_state().requires_grad and \
                not (self.lanelet_map is None or all(m is None for m in self.lanelet_map)):
            return self._compute_wrong_way(differentiable=True)
        return self._beside_render(self._compute_wrong_way, ('wrong_way',))

    def _compute_wrong_way(self, differentiable: bool = False) -> Tensor:
        state = self.get_state()
        if self.lanelet_map is None or all(m is None for m in self.lanelet_map):
            return torch.zeros(state.shape[0], state.shape[1], device=state.device)
        tol = self.cfg.lanelet_inclusion_tolerance
        assert self.cfg.wrong_way_angle_threshold >= np.pi / 2, 'direction_angle_threshold smaller than pi / 2 will produce false positives'
        fn = _ops.wrong_way_grad if differentiable else _ops.wrong_way
        return fn(self._lane_tables(state.device), state, self.recenter_offset, self.get_present_mask(), self.cfg.wrong_way_angle_threshold, tol)

    def compute_traffic_lights_violations(self) -> Tensor:
        """BxA: the agent is (mostly) past the stop line of a red light (simulator.py:1046-1062)."""
        state = self.get_state()
        controls = self.get_traffic_controls()
        if controls is not None and 'traffic_light' in controls:
            boxes = torch.cat([state[..., :2], self.get_agent_size()[..., :2], state[..., 2:3]], dim=-1)
            return controls['traffic_light'].compute_violation(boxes) * self.get_present_mask().to(state.dtype)
        return torch.zeros(state.shape[0], state.shape[1], dtype=torch.bool, device=state.device)

    def _all_boxes(self):
        return _ops.state_boxes(self.get_all_agent_state(), self.get_all_agent_size())

    def _collision_mask(self, agent_types: Optional[List[str]]):
        mask = self.get_all_agent_present_mask()
        if agent_types is not None:
            allowed = torch.tensor([self.agent_types.index(t) for t in agent_types if t in self.agent_types], device=mask.device)
            mask = mask.logical_and(torch.isin(self.get_all_agent_type(), allowed))
        return mask

    def compute_collision(self, agent_types: Optional[List[str]] = None) -> Tensor:
        """BxA collision metric of the exposed agents against ALL agents (simulator.py:1161-1194).  For `iou` / `discs`:
        collision_i = sum_j o_ij present_j - max_j o_ij present_j, self overlap assumed to be the max."""
        return self._beside_render(lambda: self._compute_collision(agent_types), ('collision', None if agent_types is None else tuple(agent_types)))

    def _compute_collision(self, agent_types: Optional[List[str]] = None) -> Tensor:
        metric = self.cfg.collision_metric
        A = self.agent_count
        if A == 0:
            return torch.zeros_like(self.get_state()[..., 0])
        if metric in (CollisionMetric.iou, CollisionMetric.discs):
            state = self.get_state()
            if self.npc_count == 0 and state.requires_grad and torch.is_grad_enabled():
                # The shared [sin, cos] node comes into being BEFORE the boxes node, as it does when render() foresees the metrics (_mark_fork
                # makes it ahead of the fork).  Autograd sums the gradients that reach a state in the order in which its consumers run, which
                # is the reverse of the order in which they were made; a state inside a rollout has four (the next step, off-road, [sin, cos],
                # boxes), three of them in the psi column, and a float sum of three depends on its order.  Made in one order on every path,
                # a rollout's gradients have the same bits with overlap_infractions on and off (tests/test_gpu_rollout.py).
                self._heading_sc()
            boxes = self._all_boxes()
            # a NaN heading is scrubbed inside the kernel, so the shared [sin, cos] of the raw headings serves the IoU metric
            sc = self._heading_sc() if metric == CollisionMetric.iou else None
            return _ops.collision(boxes, self._collision_mask(agent_types), n_exposed=A, metric=metric.value, sc=sc)
        if metric == CollisionMetric.nograd:
            assert agent_types is None, 'The argument `agent_types` is not supported by the selected collision metric.'
            # count of other present exposed agents whose rectangle shares area with the agent's (simulator.py:1111-1149 ->
            # infractions.py:352-375, where shapely answers `intersection(...).area != 0` on the host): one kernel, exact predicate in
            # float64 on the float32 corners of infractions.rectangle_vertices; NPCs are not counted, as in the reference (:1124)
            state, size, present = self.get_state().detach(), self.get_agent_size(), self.get_present_mask()
            boxes = torch.cat([state[..., :2], size, state[..., 2:3]], dim=-1)
            return _ops.overlap_count(boxes, present)
        raise ValueError('Unrecognized collision metric: ' + str(metric))
