"""
Lane-following NPC traffic: NPCs on rails along the lane centre lines, their speed set by the Intelligent Driver Model (Treiber, Hennecke,
Helbing, "Congested traffic states in empirical observations and microscopic simulations", Phys. Rev. E 62, 2000).  No reference
counterpart -- the reference's only reactive controller is an HTTP client --, so the definition is this project's own (DESIGN.md 5.5c,
include/tdship.h) and its yardstick is the float64 model tests/lane_follow_model.py.

A step of ALL NPCs of a batch is ONE kernel launch (csrc/follow.hip, `tds_lane_follow_step_multi`): every NPC looks along its path on the lane
graph -- its own lanelet, then successors chosen by a counter-based random stream keyed by `(seed, scene id, NPC index, hop)` --, finds the
nearest entity or red stop line on it, and moves by what the IDM allows.  Every NPC reads the scene as it was before the step.  State and
outputs live in buffers the controller owns and the kernel updates in place, so a `Simulator.step` with this controller can be captured
into a HIP graph; a row depends on `(seed, scene id, NPC index)` and the inputs only, so shards and sub-batches reproduce the whole batch.

With `give_way=True` the step is TWO launches: a yield pass (csrc/conflicts.hip, `tds_lane_give_way_multi`) first decides, per NPC,
whether and where it must stop before the next junction -- from a per-map table of the lanelets whose centre lines cross or merge, built once on
the device --, and the follow kernel treats that stop as one more standing obstacle.  A scene's decisions depend on that scene only.
"""
from typing import List, Optional, Sequence, Union

import torch
from torch import Tensor

from torchdrivesim_amd import _ops
from torchdrivesim_amd.lanelet2 import LaneletMap, lane_set_for
from torchdrivesim_amd.simulator import CompoundNPCController, NPCController, SpawnController, _enlarge

# IDM defaults: time headway T [s], standstill gap s0 [m], acceleration a, comfortable braking b, hardest braking b_max [m/s^2]
TIME_HEADWAY, MIN_GAP, MAX_ACCELERATION, COMFORTABLE_BRAKING, MAX_BRAKING = 1.5, 2.0, 1.5, 2.0, 6.0
DESIRED_SPEED, HORIZON, LATERAL_MARGIN = 8.0, 60.0, 0.2
CLEARANCE, CONFLICT_STEP, CREEP_SPEED = 2.0, 0.5, 1.0     # giving way: metres between centre lines, metres between samples, m/s


def _require_gpu(name: str, t: Optional[Tensor]) -> None:
    if t is not None and not t.is_cuda:
        raise RuntimeError(f'{name}: lane-following NPCs run on an MI355X; got a {t.device} tensor (no CPU fallback)')


class LaneFollowingNPCController(NPCController):
    """
    Args:
        lanelet_maps: one `LaneletMap` for all scenes or a list of B of them (the convention of `Simulator(lanelet_map=...)`)
        npc_size, npc_state, npc_present_mask: (B, N, 2), (B, N, 4) = [x, y, psi, speed], (B, N) -- e.g. from `heuristic_initialize_batch`
        seed: key of the route stream; scene_ids: (B,) int64, default arange(B): the identity of each scene in it
        desired_speed: v0 of the IDM, a number or (B, N), > 0 (checked here; a row whose value is later set to something else stands still);
            idm: (T, s0, a, b, b_max)
        obey_traffic_lights: the stop lines of `simulator.traffic_controls['traffic_light']` whose state is `red` stand on the road as boxes
        tolerance: of the one `snap_to_lanes` call that puts the states onto lanes; NPCs that find no lane (`lane == -1`) stay where they are
        give_way: NPCs give way to each other at junctions (off: the launches, buffers and bits are those of a controller without the option).
            clearance, conflict_step: two lanelets conflict where their centre lines, sampled every `conflict_step` metres, come within
            `clearance` metres (the tables are built here, once per map); creep_speed: the least speed an NPC's time to the junction is
            reckoned with.  Who goes first: an NPC that can no longer stop, else the one that is there sooner, the lower index on a tie; nobody
            waits for an NPC held by a red light (with `obey_traffic_lights`: the stop lines are put onto lanes once, at the first step).
            At most 1024 NPCs per scene.  Exposed agents are no contenders (they have no path; an NPC still brakes for one in its way).
    As a member of the simulator's `CompoundNPCController` it moves the rows that `controller_indices` gives it and no others.  NPCs that its
    `SpawnController` puts somewhere else are snapped to the lane under their new pose (not inside a compound, where spawning acts on the
    compound's tensors).
    Per NPC the controller exposes `lane` (int32 index into `laneletLayer`), `arc` (float64, metres along its centre line), `hops` (int32,
    lanelet transitions so far) and `leader` (int32: the entity row braked for in the last step, -1 none, -2 the end of the lane, -3 the
    junction it gives way at); with `give_way` also `stop_at` (float64: the path distance at which it had to stop in the last step, +inf none)
    and `yield_to` (int32: the NPC index it gave way to, -1 none).  As a member of a `CompoundNPCController` a controller contends with its own
    rows only: NPCs of other members are obstacles on its path like any entity, not contenders at a junction.
    """

    def __init__(self, lanelet_maps: Union[LaneletMap, Sequence[Optional[LaneletMap]]], npc_size: Tensor, npc_state: Tensor,
                 npc_present_mask: Optional[Tensor] = None, *, seed: int, scene_ids: Optional[Tensor] = None,
                 desired_speed: Union[float, Tensor] = DESIRED_SPEED, idm=(TIME_HEADWAY, MIN_GAP, MAX_ACCELERATION, COMFORTABLE_BRAKING, MAX_BRAKING),
                 horizon: float = HORIZON, lateral_margin: float = LATERAL_MARGIN, obey_traffic_lights: bool = True, tolerance: float = 1.0,
                 npc_types: Optional[Tensor] = None, agent_type_names: Optional[List[str]] = None,
                 spawn_controller: Optional[SpawnController] = None, give_way: bool = False, clearance: float = CLEARANCE,
                 conflict_step: float = CONFLICT_STEP, creep_speed: float = CREEP_SPEED, _snapped=None):
        for name, t in (('npc_size', npc_size), ('npc_state', npc_state), ('npc_present_mask', npc_present_mask), ('scene_ids', scene_ids),
                        ('desired_speed', desired_speed if isinstance(desired_speed, Tensor) else None)):
            _require_gpu(name, t)
        if npc_state.dim() != 3 or npc_state.shape[-1] != 4:
            raise ValueError(f'npc_state must be (B, N, 4), got {tuple(npc_state.shape)}')
        B, N = npc_state.shape[:2]
        dev = npc_state.device
        _ops.check_lane_follow_args(0, 0.0, horizon, lateral_margin, idm)
        self.give_way, self.clearance, self.conflict_step, self.creep_speed = bool(give_way), float(clearance), float(conflict_step), float(creep_speed)
        if self.give_way:
            _ops.check_lane_conflicts_args(0, self.clearance, self.conflict_step)
            _ops.check_lane_give_way_args(N, horizon, idm[4], self.creep_speed)
        super().__init__(npc_size, npc_state.detach().to(torch.float32).clone(), npc_present_mask, npc_types, agent_type_names, spawn_controller)
        self.lanelet_maps = lanelet_maps if isinstance(lanelet_maps, LaneletMap) else list(lanelet_maps)
        self.seed, self.idm, self.horizon, self.lateral_margin = int(seed), tuple(float(x) for x in idm), float(horizon), float(lateral_margin)
        self.obey_traffic_lights, self.tolerance = bool(obey_traffic_lights), float(tolerance)
        self.scene_ids = torch.arange(B, dtype=torch.int64, device=dev) if scene_ids is None else scene_ids.to(torch.int64).clone()
        if isinstance(desired_speed, Tensor):
            self.desired_speed = desired_speed.to(torch.float32).expand(B, N).clone()
            if B * N > 0 and not bool((self.desired_speed > 0).all()):
                raise ValueError('desired_speed must be > 0 for every NPC')
        elif not float(desired_speed) > 0:
            raise ValueError(f'desired_speed must be > 0, got {desired_speed}')
        else:
            self.desired_speed = torch.full((B, N), float(desired_speed), dtype=torch.float32, device=dev)
        self._lanes = None
        if _snapped is None:
            from torchdrivesim_amd.lanelet2 import snap_to_lanes
            self.lane, self.arc, _ = snap_to_lanes(self.lanelet_maps, self.npc_state, self.tolerance)
            self.hops = torch.zeros((B, N), dtype=torch.int32, device=dev)
            self.leader = torch.full((B, N), -1, dtype=torch.int32, device=dev)
            self.npc_sc = _ops.heading_sc(self.npc_state[..., 2])
        else:
            self.lane, self.arc, self.hops, self.leader, self.npc_sc = (t.clone() for t in _snapped)
        self._self_index = None
        self._state_buffer = self.npc_state
        self.stop_at = self.yield_to = self._conflicts = self._lines = None
        if self.give_way:
            self.stop_at = torch.full((B, N), float('inf'), dtype=torch.float64, device=dev)
            self.yield_to = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        self._lane_table_set()

    # ---- plumbing ---------------------------------------------------------------------------------------------------------------
    def _lane_table_set(self):
        """the device lane tables of this batch: found (or built) outside the step, so that the step allocates and copies nothing"""
        if self._lanes is None and self.npc_state.shape[0] > 0:
            self._lanes = lane_set_for(self.lanelet_maps, self.npc_state.shape[0], self.npc_state.device)
            if self.give_way:                                              # built once per map, kept on its lane table
                self._conflicts = self._lanes.conflict_tables(self.clearance, self.conflict_step)
        return self._lanes

    def _map(self, f):
        self.lane, self.arc, self.hops, self.leader, self.npc_sc = f(self.lane), f(self.arc), f(self.hops), f(self.leader), f(self.npc_sc)
        self.scene_ids, self.desired_speed = f(self.scene_ids), f(self.desired_speed)
        super()._map(f)
        # the kernel updates these in place: dense tensors of its own types, owned by this controller
        self.npc_state = self._state_buffer = self.npc_state.to(torch.float32).contiguous()
        self.lane, self.arc, self.hops = self.lane.contiguous(), self.arc.contiguous(), self.hops.contiguous()
        self.leader, self.npc_sc = self.leader.contiguous(), self.npc_sc.contiguous()
        if self.give_way:
            self.stop_at, self.yield_to = f(self.stop_at).contiguous(), f(self.yield_to).contiguous()
        self._lanes = self._self_index = self._conflicts = self._lines = None
        self._lane_table_set()
        return self

    def copy(self):
        new = self.__class__(self.lanelet_maps, self.npc_size, self.npc_state, self.npc_present_mask, seed=self.seed, scene_ids=self.scene_ids,
                             desired_speed=self.desired_speed, idm=self.idm, horizon=self.horizon, lateral_margin=self.lateral_margin,
                             obey_traffic_lights=self.obey_traffic_lights, tolerance=self.tolerance, npc_types=self.npc_types,
                             agent_type_names=self.agent_type_names, spawn_controller=self.spawn_controller.copy(), give_way=self.give_way,
                             clearance=self.clearance, conflict_step=self.conflict_step, creep_speed=self.creep_speed,
                             _snapped=(self.lane, self.arc, self.hops, self.leader, self.npc_sc))
        if self.give_way:                                                  # what the last step decided goes with the copy
            new.stop_at.copy_(self.stop_at), new.yield_to.copy_(self.yield_to)
        return new

    def extend(self, n, in_place=True):
        me = self if in_place else self.copy()
        if not isinstance(me.lanelet_maps, LaneletMap):
            me.lanelet_maps = [m for m in me.lanelet_maps for _ in range(n)]
        me.spawn_controller.extend(n, in_place=True)
        return me._map(lambda x: _enlarge(x, n))

    def select_batch_elements(self, idx, in_place=True):
        me = self if in_place else self.copy()
        if not isinstance(me.lanelet_maps, LaneletMap):
            me.lanelet_maps = [me.lanelet_maps[int(i)] for i in idx]
        me.spawn_controller.select_batch_elements(idx, in_place=True)
        return me._map(lambda x: x[idx])

    # ---- the step -----------------------------------------------------------------------------------------------------------------
    def _entities(self, simulator):
        """(boxes (B,E,5), [sin, cos] (B,E,2), speed (B,E), present (B,E)) of everything an NPC may have to brake for: all agents and NPCs of the
        simulator, then the red stop lines as standing boxes"""
        state, size = simulator.get_all_agent_state().detach(), simulator.get_all_agent_size()
        boxes = torch.cat([state[..., :2], size, state[..., 2:3]], dim=-1)
        sc, speed, present = simulator._heading_sc().detach(), state[..., 3], simulator.get_all_agent_present_mask()
        lights = (simulator.traffic_controls or {}).get('traffic_light') if self.obey_traffic_lights else None
        if lights is not None and lights.pos.shape[1] > 0:
            pos = lights.pos.to(boxes.dtype)
            red = (lights.state == lights.allowed_states.index('red')) & lights.mask
            boxes, sc = torch.cat([boxes, pos], dim=1), torch.cat([sc, _ops.heading_sc(pos[..., 4])], dim=1)
            speed, present = torch.cat([speed, torch.zeros_like(pos[..., 0])], dim=1), torch.cat([present, red], dim=1)
        return boxes, sc, speed.contiguous(), present

    def _stop_lines(self, simulator):
        """None, or (line_lane (B,S) int32, line_arc (B,S) float64, line_red (B,S) bool) of the traffic lights' stop lines: put onto lanes once per
        `traffic_light` control with `snap_to_lanes` (a line that finds no lane has lane -1 and holds nobody), red as the lights stand now"""
        lights = (simulator.traffic_controls or {}).get('traffic_light') if self.obey_traffic_lights else None
        if lights is None or lights.pos.shape[1] == 0:
            return None
        if self._lines is None or self._lines[0] is not lights or self._lines[1] is not lights.pos:
            from torchdrivesim_amd.lanelet2 import snap_to_lanes
            pos = lights.pos.to(torch.float32)
            pose = torch.stack([pos[..., 0], pos[..., 1], pos[..., 4], torch.zeros_like(pos[..., 0])], dim=-1)
            lane, arc, _ = snap_to_lanes(self.lanelet_maps, pose, self.tolerance)
            self._lines = (lights, lights.pos, lane, arc)
        red = (lights.state == lights.allowed_states.index('red')) & lights.mask
        return self._lines[2], self._lines[3], red

    def _own_state(self) -> None:
        """The kernel writes the state in place, so it writes a buffer of THIS controller only.  A tensor that was handed in since the last step --
        the merged state a `CompoundNPCController` gives to all its members, a `SpawnController`'s result -- is copied into that buffer first."""
        if self.npc_state is not self._state_buffer:
            if self._state_buffer.shape == self.npc_state.shape and self._state_buffer.device == self.npc_state.device:
                self._state_buffer.copy_(self.npc_state)
            else:
                self._state_buffer = self.npc_state.detach().to(torch.float32).clone()
            self.npc_state = self._state_buffer

    def _rows_to_move(self, simulator) -> Tensor:
        """present rows; as a member of the simulator's `CompoundNPCController`, the present rows this controller owns there"""
        top = simulator.npc_controller
        if isinstance(top, CompoundNPCController):
            for i, member in enumerate(top.controllers):
                if member is self:
                    return self.npc_present_mask & (top.controller_indices == i)
        return self.npc_present_mask

    def _snap_spawned(self, spawned: Tensor) -> None:
        """rows a `SpawnController` has just put somewhere else start from the lane under their new pose"""
        from torchdrivesim_amd.lanelet2 import snap_to_lanes
        lane, arc, _ = snap_to_lanes(self.lanelet_maps, self.npc_state, self.tolerance)
        self.lane.copy_(torch.where(spawned, lane, self.lane))
        self.arc.copy_(torch.where(spawned, arc, self.arc))
        self.hops.copy_(torch.where(spawned, torch.zeros_like(self.hops), self.hops))
        self.npc_sc.copy_(torch.where(spawned.unsqueeze(-1), _ops.heading_sc(self.npc_state[..., 2]), self.npc_sc))

    def advance_npcs(self, simulator) -> None:
        _require_gpu('npc_state', self.npc_state)
        B, N = self.npc_state.shape[:2]
        if B * N > 0:
            with torch.no_grad():
                self._own_state()
                boxes, sc, speed, present = self._entities(simulator)
                # the NPCs of this controller are the simulator's NPC rows, behind the exposed agents
                A = simulator.agent_count
                if self._self_index is None or self._self_index[0] != A:
                    rows = torch.arange(A, A + N, dtype=torch.int32, device=self.npc_state.device)
                    self._self_index = (A, rows.unsqueeze(0).expand(B, N).contiguous())
                lanes, rows_to_move = self._lane_table_set(), self._rows_to_move(simulator)
                if self.give_way:
                    _ops.lane_give_way(lanes, self.scene_ids, self._conflicts, self.lane, self.arc, self.hops, self.npc_state, self.npc_size, rows_to_move,
                                       self._stop_lines(simulator), self.seed, self.stop_at, self.yield_to, self.horizon, self.idm[4], self.creep_speed)
                _ops.lane_follow_step(lanes, self.scene_ids, boxes, sc, speed, present, self._self_index[1], self.npc_size,
                                      self.desired_speed, rows_to_move, self.lane, self.arc, self.hops, self.npc_state, self.npc_sc,
                                      self.leader, self.seed, simulator.kinematic_model.dt, self.horizon, self.lateral_margin, self.idm,
                                      stop_at=self.stop_at)
        was_present = self.npc_present_mask
        self.spawn_despawn_npcs(simulator)
        if self.spawn_controller.spawn_states is not None and simulator.npc_controller is self and B * N > 0:
            with torch.no_grad():
                self._own_state()
                self._snap_spawned(self.npc_present_mask & ~was_present)
