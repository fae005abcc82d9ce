"""
Waypoint goals with the reference's surface (torchdrivesim/goals.py:11-217): every agent has `N` successive collections of `M`
waypoints; the collection `state[b, a]` is current, and it is ticked off as soon as the agent comes within `threshold` of any of its
(valid) waypoints.  Host-side torch bookkeeping on small tensors -- no kernel of its own; the waypoints of the current
collections are drawn by the K3 rasteriser as per-camera discs (`Simulator.render`, mesh.py:1120-1145 in the reference).

Route goals (`RouteGoal`, no reference counterpart; DESIGN.md 5.5d, csrc/route.hip): every agent is dealt a route of a requested length on the
lane graph; each step ONE launch reports its progress along it, its offsets from it, whether it has arrived or left it, and the next K route
points in its own frame.  Yardstick: the float64 model tests/route_model.py.  `RouteGoal.to` deals the shortest route to a destination instead
of a random one (csrc/route_to.hip; model: tests/route_to_model.py).  With `differentiable=True` the step's float outputs carry
gradients to the pose, one backward launch (csrc/route_bwd.hip; model: tests/route_grad_model.py).
"""
from typing import NamedTuple, Optional, Union

import torch
from torch import Tensor


class WaypointGoal:
    """waypoints: B x A x N x M x 2 (x, y); mask: B x A x N x M bool, False = padding (default: all True)."""

    def __init__(self, waypoints: Tensor, mask: Optional[Tensor] = None):
        self.waypoints = waypoints
        self.mask = mask if mask is not None else torch.ones(waypoints.shape[:-1], dtype=torch.bool, device=waypoints.device)
        self.max_goal_idx = waypoints.shape[2]
        self.state = torch.zeros(waypoints.shape[:2] + (1,), dtype=torch.long, device=waypoints.device)      # B x A x 1

    # ---- the `count` collections starting at the current one, flattened to count*M; collections past the end are zeros / False
    def _window(self, count: int):
        idx = self.state + torch.arange(count, device=self.state.device).view(1, 1, -1)                       # B x A x count
        return idx.clamp(0, self.max_goal_idx - 1), idx < self.max_goal_idx

    def get_masks(self, count: int = 1) -> Tensor:
        """B x A x count*M (goals.py:33-69)"""
        idx, valid = self._window(count)
        M = self.mask.shape[3]
        got = torch.gather(self.mask, 2, idx[..., None].expand(-1, -1, -1, M)) & valid[..., None]
        return got.reshape(got.shape[:2] + (count * M,))

    def get_waypoints(self, count: int = 1) -> Tensor:
        """B x A x count*M x 2 (goals.py:71-107)"""
        idx, valid = self._window(count)
        M = self.waypoints.shape[3]
        got = torch.gather(self.waypoints, 2, idx[..., None, None].expand(-1, -1, -1, M, 2))
        got = torch.where(valid[..., None, None], got, torch.zeros_like(got))
        return got.reshape(got.shape[:2] + (count * M, 2))

    # ---- batch plumbing (goals.py:109-160)
    def copy(self):
        other = self.__class__(waypoints=self.waypoints.clone(), mask=self.mask.clone())
        other.state = self.state.clone()
        return other

    def to(self, device):
        self.waypoints, self.mask, self.state = self.waypoints.to(device), self.mask.to(device), self.state.to(device)
        return self

    def extend(self, n: int, in_place: bool = True):
        target = self if in_place else self.copy()
        rep = lambda x: x.unsqueeze(1).expand((x.shape[0], n) + x.shape[1:]).reshape((n * x.shape[0],) + x.shape[1:])
        target.waypoints, target.mask, target.state = rep(target.waypoints), rep(target.mask), rep(target.state)
        return target

    def select_batch_elements(self, idx, in_place: bool = True):
        target = self if in_place else self.copy()
        target.waypoints, target.mask, target.state = target.waypoints[idx], target.mask[idx], target.state[idx]
        return target

    def step(self, agent_states: Tensor, time: int = 0, threshold: float = 2.0) -> None:
        """Tick off the current collection of every agent that is within `threshold` of one of its valid waypoints: its valid
        entries become False and the state moves on, saturating at the last collection (goals.py:162-217)."""
        assert agent_states.shape[1] == self.waypoints.shape[1]
        wp, valid = self.get_waypoints(), self.get_masks()                               # B x A x M (x 2)
        dx, dy = agent_states[..., None, 0] - wp[..., 0], agent_states[..., None, 1] - wp[..., 1]
        near = ((dx ** 2) + (dy ** 2)) ** 0.5 <= threshold
        reached = (near & valid).any(dim=-1, keepdim=True)                               # B x A x 1
        idx = self.state[..., None].expand(-1, -1, -1, self.mask.shape[-1])              # B x A x 1 x M
        self.mask = self.mask.scatter(2, idx, (valid & ~reached).unsqueeze(2))           # padding entries stay False
        self.state = (self.state + reached).clamp(0, self.max_goal_idx - 1)


class RouteProgress(NamedTuple):
    """What one `RouteGoal.step` reports, (B, A) each unless said otherwise; float32 and bool.  The tensors are buffers of the goal object:
    the next step overwrites them in place (clone what has to outlive it)."""
    progress: Tensor       # metres along the route
    advance: Tensor        # progress minus the progress of the previous step
    lateral: Tensor        # signed offset from the route, left positive
    heading: Tensor        # (B, A, 2) [sin, cos] of the heading error against the route's direction
    remaining: Tensor      # length - progress
    reached: Tensor        # remaining <= goal_tolerance
    off_route: Tensor      # farther than off_route_distance from the route
    lookahead: Tensor      # (B, A, K, 2) the route points at progress + (m + 1) * spacing in the agent's frame


_ROUTE_OUT = (('progress', ()), ('advance', ()), ('lateral', ()), ('heading', (2,)), ('remaining', ()), ('reached', ()), ('off_route', ()))


class _ClassOrInstance:
    """`RouteGoal.to(...)` on the class deals routes to destinations; `goal.to(device)` on an object moves it, as on every goal object"""

    def __init__(self, on_class, on_instance):
        self.on_class, self.on_instance = on_class, on_instance
        self.__doc__ = on_class.__doc__

    def __get__(self, obj, cls):
        return self.on_class.__get__(None, cls) if obj is None else self.on_instance.__get__(obj, cls)


class RouteGoal:
    """
    Routes on the lane graph, one per agent, and the per-step bookkeeping of them on the device (include/tdship.h "Route goals").
    Make one with `RouteGoal.sample` (a random route of a requested length) or `RouteGoal.to` (the shortest route to a destination).  Per agent it
    exposes `lanes` (B, A, 16) int32 (indices into `laneletLayer`, -1 unused), `n` (B, A) int32, `start_arc`, `end_arc`, `offsets` (B, A, 16), `length` (float64), `cursor` (int32), `completed` and `valid` (bool).  A row depends on
    `(seed, scene id, agent index)` and its own pose only, so shards and sub-batches reproduce the whole batch.
    """

    def __init__(self, lanelet_maps, tensors: dict, *, seed: int, tolerance: float, goal_tolerance: float, off_route_distance: float, lookahead: int,
                 spacing: float, differentiable: bool = False):
        from torchdrivesim_amd import _ops
        from torchdrivesim_amd.lanelet2 import LaneletMap
        _ops.check_route_args(goal_tolerance, off_route_distance, lookahead, spacing)
        self.lanelet_maps = lanelet_maps if isinstance(lanelet_maps, LaneletMap) else list(lanelet_maps)
        self.seed, self.tolerance, self.goal_tolerance = int(seed), float(tolerance), float(goal_tolerance)
        self.off_route_distance, self.lookahead, self.spacing = float(off_route_distance), int(lookahead), float(spacing)
        self.differentiable = bool(differentiable)       # `step` returns float outputs that carry the graph to the pose; settable
        self._t = dict(tensors)       # the route tensors, its state, the requested lengths, the scene ids, scratch of the snap and the outputs
        self._lanes = None
        self._lane_table_set()

    # ---- construction -------------------------------------------------------------------------------------------------------------
    @classmethod
    def sample(cls, lanelet_maps, agent_state: Tensor, present_mask: Optional[Tensor] = None, *, seed: int, scene_ids: Optional[Tensor] = None,
               length: Union[float, Tensor] = 200.0, tolerance: float = 1.0, goal_tolerance: float = 2.0, off_route_distance: float = 4.0,
               lookahead: int = 16, spacing: float = 4.0, differentiable: bool = False) -> 'RouteGoal':
        """
        lanelet_maps: one `LaneletMap` for all scenes or a list of B of them; agent_state (B, A, >= 3) = [x, y, psi, ...] on the device.
        Every present agent is snapped to a lane (`snap_to_lanes` with `tolerance`) and dealt a route of `length` metres (a number or (B, A))
        from there; agents that find no lane, absent ones and lengths that are not positive and finite get no route (`valid` False).
        seed: key of the route stream; scene_ids (B,) int64, default arange(B): the identity of each scene in it.
        differentiable: `step` hands out float outputs with gradients to the pose (see `step`).
        """
        from torchdrivesim_amd import _ops
        for name, t in (('agent_state', agent_state), ('present_mask', present_mask), ('scene_ids', scene_ids),
                        ('length', length if isinstance(length, Tensor) else None)):
            if t is not None and not t.is_cuda:
                raise RuntimeError(f'{name}: route goals run on an MI355X; got a {t.device} tensor (no CPU fallback)')
        if agent_state.dim() != 3 or agent_state.shape[-1] < 3:
            raise ValueError(f'agent_state must be (B, A, >= 3), got {tuple(agent_state.shape)}')
        B, A = agent_state.shape[:2]
        dev = agent_state.device
        K = int(lookahead)
        _ops.check_route_args(goal_tolerance, off_route_distance, K, spacing)
        f64 = torch.float64
        t = cls._buffers(B, A, K, dev)
        t['scene_ids'] = torch.arange(B, dtype=torch.int64, device=dev) if scene_ids is None else scene_ids.to(torch.int64).clone()
        if isinstance(length, Tensor):
            t['distance'] = length.to(f64).expand(B, A).clone()
        else:
            t['distance'] = torch.full((B, A), float(length), dtype=f64, device=dev)
        me = cls(lanelet_maps, t, seed=seed, tolerance=tolerance, goal_tolerance=goal_tolerance, off_route_distance=off_route_distance, lookahead=K,
                 spacing=spacing, differentiable=differentiable)
        me._sample(agent_state, present_mask, None)
        return me

    @staticmethod
    def _buffers(B, A, K, dev) -> dict:
        """what every route goal holds: the route tensors, their state, the outputs of a step and what a snap reads and writes (kept, so that
        dealing new routes allocates nothing)"""
        from torchdrivesim_amd import _ops
        f32, f64, i32, u8 = torch.float32, torch.float64, torch.int32, torch.uint8
        t = {name: torch.zeros((B, A) + tail, dtype=dtype, device=dev) for name, tail, dtype in _ops.ROUTE_TENSORS + _ops.ROUTE_STATE}
        t.update({name: torch.zeros((B, A) + tail, dtype=u8 if name in ('reached', 'off_route') else f32, device=dev) for name, tail in _ROUTE_OUT})
        t['lookahead'] = torch.zeros((B, A, K, 2), dtype=f32, device=dev)
        t.update(snap_xy=torch.zeros((B, A, 2), dtype=f32, device=dev), sc=torch.zeros((B, A, 2), dtype=f32, device=dev),
                 snap_lane=torch.zeros((B, A), dtype=i32, device=dev), snap_arc=torch.zeros((B, A), dtype=f64, device=dev),
                 snap_lateral=torch.zeros((B, A), dtype=f32, device=dev))
        return t

    @classmethod
    def _to_destination(cls, lanelet_maps, agent_state: Tensor, destination: Optional[Tensor] = None, *, destination_lanes: Optional[Tensor] = None,
                        destination_arcs: Optional[Tensor] = None, present_mask: Optional[Tensor] = None, tolerance: float = 1.0,
                        goal_tolerance: float = 2.0, off_route_distance: float = 4.0, lookahead: int = 16, spacing: float = 4.0,
                        differentiable: bool = False) -> 'RouteGoal':
        """
        RouteGoal.to(lanelet_maps, agent_state, destination): the SHORTEST route on the lane graph from every agent to its destination.
        lanelet_maps, agent_state, tolerance and the step's parameters: as for `sample`.  The destination is given in exactly one of two forms:
        `destination` (B, A, 3) poses [x, y, psi], snapped to a lane like the agents (`snap_to_lanes` with `tolerance`), or `destination_lanes`
        (B, A) int lanelet indices with `destination_arcs` (B, A) arc lengths on them.  Agents and destinations that find no lane, absent agents and
        destinations that cannot be reached get no route (`valid` False, `rest` inf).  A route holds at most 16 lanelets: one that would need
        more ends at the end of its 16th (`truncated`; `rest` = what is left from there) and is continued with
        `resample_to(state, mask=goal.completed & goal.truncated)`.  The first call with a map builds its distance tables (L x L float64, one
        launch): outside any stream capture.  No lane changes, no cost but length.  differentiable: as for `sample`.
        """
        from torchdrivesim_amd import _ops
        if not agent_state.is_cuda:
            raise RuntimeError(f'agent_state: route goals run on an MI355X; got a {agent_state.device} tensor (no CPU fallback)')
        if agent_state.dim() != 3 or agent_state.shape[-1] < 3:
            raise ValueError(f'agent_state must be (B, A, >= 3), got {tuple(agent_state.shape)}')
        B, A = agent_state.shape[:2]
        K = int(lookahead)
        _ops.check_route_args(goal_tolerance, off_route_distance, K, spacing)
        if destination is None and destination_lanes is None:
            raise ValueError('RouteGoal.to needs `destination` poses or `destination_lanes` and `destination_arcs`')
        me = cls(lanelet_maps, cls._buffers(B, A, K, agent_state.device), seed=0, tolerance=tolerance, goal_tolerance=goal_tolerance,
                 off_route_distance=off_route_distance, lookahead=K, spacing=spacing, differentiable=differentiable)
        me.resample_to(agent_state, destination, present_mask=present_mask, destination_lanes=destination_lanes, destination_arcs=destination_arcs)
        return me

    def _lane_table_set(self):
        """the device lane tables of this batch: found (or built) outside the step, so that the step allocates and copies nothing"""
        from torchdrivesim_amd.lanelet2 import lane_set_for
        n = self._t['n']
        if self._lanes is None and n.shape[0] > 0:
            self._lanes = lane_set_for(self.lanelet_maps, n.shape[0], n.device)
        return self._lanes

    def _heading(self, agent_state: Tensor, into: str = 'sc') -> Tensor:
        """[sin, cos] of the headings with torch, into the buffer this object keeps for them"""
        psi = agent_state[..., 2].detach()
        torch.sin(psi, out=self._t[into][..., 0])
        torch.cos(psi, out=self._t[into][..., 1])
        return self._t[into]

    def _sample(self, agent_state, present_mask, mask) -> None:
        from torchdrivesim_amd import _ops
        t = self._t
        if 'distance' not in t:
            raise RuntimeError('this RouteGoal was made by RouteGoal.to: it has no requested lengths to sample routes of (use resample_to)')
        B, A = t['n'].shape
        if tuple(agent_state.shape[:2]) != (B, A):
            raise ValueError(f'agent_state must be ({B}, {A}, >= 3), got {tuple(agent_state.shape)}')
        if B * A == 0:
            return
        with torch.no_grad():
            t['snap_xy'].copy_(agent_state[..., :2])
            _ops.lane_snap(self._lane_table_set(), t['snap_xy'], self._heading(agent_state), self.tolerance,
                           out=(t['snap_lane'], t['snap_arc'], t['snap_lateral']))
            _ops.route_sample(self._lane_table_set(), t['scene_ids'], t['snap_lane'], t['snap_arc'], t['distance'], present_mask, mask, self.seed, t)

    def resample(self, agent_state: Tensor, scene_ids: Optional[Tensor] = None, mask: Optional[Tensor] = None, present_mask: Optional[Tensor] = None) -> None:
        """New routes IN PLACE from where the agents are now -- all rows, or the rows of `mask` (B, A) bool; the others keep route, cursor and
        `completed`.  scene_ids (B,): the scenes' new identities in the route stream (a reset usually moves on to fresh ones).  Two launches and
        the copies into this object's buffers; nothing is allocated, nothing synchronises."""
        if not agent_state.is_cuda:
            raise RuntimeError(f'agent_state: route goals run on an MI355X; got a {agent_state.device} tensor (no CPU fallback)')
        if scene_ids is not None:
            self._t['scene_ids'].copy_(scene_ids)
        self._sample(agent_state, present_mask, mask)

    def _set_destinations(self, destination, lanes, arcs, mask) -> None:
        """the stored destinations of all rows, or of the rows of `mask`, from poses or from (lane, arc); without either they must exist"""
        t = self._t
        B, A = t['n'].shape
        if (destination is not None) == (lanes is not None) or (lanes is None) != (arcs is None):
            if destination is None and lanes is None and arcs is None:
                if 'dest_lane' not in t:
                    raise RuntimeError('this RouteGoal has no stored destinations (it was made by RouteGoal.sample): give `destination` or '
                                       '`destination_lanes` and `destination_arcs`')
                return
            raise ValueError('give either `destination` poses or both `destination_lanes` and `destination_arcs`')
        for name, x in (('destination', destination), ('destination_lanes', lanes), ('destination_arcs', arcs), ('mask', mask)):
            if x is not None and not x.is_cuda:
                raise RuntimeError(f'{name}: route goals run on an MI355X; got a {x.device} tensor (no CPU fallback)')
        if 'dest_lane' not in t:                                             # the first destinations of this object: its buffers for them
            dev, f32 = t['n'].device, torch.float32
            t.update(dest_lane=torch.full((B, A), -1, dtype=torch.int32, device=dev), dest_arc=torch.zeros((B, A), dtype=torch.float64, device=dev),
                     rest=torch.full((B, A), float('inf'), dtype=torch.float64, device=dev), dest_xy=torch.zeros((B, A, 2), dtype=f32, device=dev),
                     dest_sc=torch.zeros((B, A, 2), dtype=f32, device=dev))
        if destination is not None:
            from torchdrivesim_amd import _ops
            if destination.dim() != 3 or tuple(destination.shape[:2]) != (B, A) or destination.shape[-1] < 3:
                raise ValueError(f'destination must be ({B}, {A}, >= 3), got {tuple(destination.shape)}')
            if B * A == 0:
                return
            t['dest_xy'].copy_(destination[..., :2])
            _ops.lane_snap(self._lane_table_set(), t['dest_xy'], self._heading(destination, 'dest_sc'), self.tolerance,
                           out=(t['snap_lane'], t['snap_arc'], t['snap_lateral']))      # (the agents' snap, which follows, overwrites these)
            lanes, arcs = t['snap_lane'], t['snap_arc']
        elif tuple(lanes.shape) != (B, A) or tuple(arcs.shape) != (B, A):
            raise ValueError(f'destination_lanes and destination_arcs must be ({B}, {A}), got {tuple(lanes.shape)}, {tuple(arcs.shape)}')
        if mask is None:
            t['dest_lane'].copy_(lanes), t['dest_arc'].copy_(arcs)
        else:                                                               # rows outside the mask keep the destination their route leads to
            torch.where(mask, lanes.to(torch.int32), t['dest_lane'], out=t['dest_lane'])
            torch.where(mask, arcs.to(torch.float64), t['dest_arc'], out=t['dest_arc'])

    def resample_to(self, agent_state: Tensor, destination: Optional[Tensor] = None, mask: Optional[Tensor] = None, present_mask: Optional[Tensor] = None, *,
                    destination_lanes: Optional[Tensor] = None, destination_arcs: Optional[Tensor] = None) -> None:
        """Shortest routes IN PLACE from where the agents are now to the stored destinations, or to new ones (`destination` poses, or
        `destination_lanes` with `destination_arcs`, as for `RouteGoal.to`) -- all rows, or the rows of `mask` (B, A) bool; the others keep route,
        destination, `rest`, cursor and `completed`.  `mask=goal.completed & goal.truncated` continues routes that were cut at 16 lanelets,
        `mask=progress.off_route` plans again for agents that have left theirs.  With the stored destinations, or with new ones in tensors of this
        object's types (int32 / float64), nothing is allocated and nothing synchronises."""
        from torchdrivesim_amd import _ops
        if not agent_state.is_cuda:
            raise RuntimeError(f'agent_state: route goals run on an MI355X; got a {agent_state.device} tensor (no CPU fallback)')
        t = self._t
        B, A = t['n'].shape
        if agent_state.dim() != 3 or tuple(agent_state.shape[:2]) != (B, A) or agent_state.shape[-1] < 3:
            raise ValueError(f'agent_state must be ({B}, {A}, >= 3), got {tuple(agent_state.shape)}')
        if mask is not None and tuple(mask.shape) != (B, A):
            raise ValueError(f'mask must be ({B}, {A}), got {tuple(mask.shape)}')
        with torch.no_grad():
            self._set_destinations(destination, destination_lanes, destination_arcs, mask)
            if B * A == 0:
                return
            t['snap_xy'].copy_(agent_state[..., :2])
            _ops.lane_snap(self._lane_table_set(), t['snap_xy'], self._heading(agent_state), self.tolerance,
                           out=(t['snap_lane'], t['snap_arc'], t['snap_lateral']))
            _ops.route_to(self._lane_table_set(), t['snap_lane'], t['snap_arc'], t['dest_lane'], t['dest_arc'], present_mask, mask, t)

    # ---- the step -----------------------------------------------------------------------------------------------------------------
    def step(self, agent_state: Tensor, present_mask: Optional[Tensor] = None, sc: Optional[Tensor] = None) -> RouteProgress:
        """One launch for all agents: agent_state (B, A, >= 3) = [x, y, psi, ...]; sc: (B, A, 2) [sin psi, cos psi] where the caller has them
        already (else computed here with torch).  Returns the `RouteProgress` of the buffers this object owns.

        With `differentiable` set, grad mode on and an `agent_state` or `sc` that requires grad, the same launch runs as an autograd node
        (`_ops.route_progress_grad`): the float fields of what is returned are CLONES that carry the graph to [x, y] and to [sin psi, cos psi]
        (computed here with `_ops.heading_sc` when not handed in, so psi gets its gradient through torch's sin / cos); the flags stay this
        object's buffers, and `last_progress` still gives the buffers.  The forward's discrete choices (piece, segment, clamps) are constants;
        `advance` differentiates as `progress` (the stored progress of the previous step is a constant: for the telescoped sum through time,
        differentiate `progress` itself).  The backward is one launch; new routes (`resample`, `resample_to`) before it make it raise."""
        from torchdrivesim_amd import _ops
        if not agent_state.is_cuda:
            raise RuntimeError(f'agent_state: route goals run on an MI355X; got a {agent_state.device} tensor (no CPU fallback)')
        t = self._t
        B, A = t['n'].shape
        if agent_state.dim() != 3 or tuple(agent_state.shape[:2]) != (B, A) or agent_state.shape[-1] < 3:
            raise ValueError(f'agent_state must be ({B}, {A}, >= 3), got {tuple(agent_state.shape)}')
        if self.differentiable and B * A > 0 and torch.is_grad_enabled() and (agent_state.requires_grad or (sc is not None and sc.requires_grad)):
            if sc is None:
                sc = _ops.heading_sc(agent_state[..., 2])
            with torch.no_grad():
                t['sc'].copy_(sc)                                            # the buffer always holds the [sin, cos] the last launch read
            f = _ops.route_progress_grad(self._lane_table_set(), agent_state, sc, present_mask, t, t, self.goal_tolerance, self.off_route_distance,
                                         self.spacing)
            return RouteProgress(f[0], f[1], f[2], f[3], f[4], t['reached'].view(torch.bool), t['off_route'].view(torch.bool), f[5])
        if B * A > 0:
            with torch.no_grad():
                if sc is None:
                    self._heading(agent_state)
                else:
                    t['sc'].copy_(sc)                                        # the buffer always holds the [sin, cos] the last launch read
                _ops.route_progress(self._lane_table_set(), agent_state, t['sc'], present_mask, t, t, self.goal_tolerance, self.off_route_distance,
                                    self.spacing)
        return self.last_progress

    @property
    def last_progress(self) -> RouteProgress:
        t = self._t
        return RouteProgress(t['progress'], t['advance'], t['lateral'], t['heading'], t['remaining'], t['reached'].view(torch.bool),
                             t['off_route'].view(torch.bool), t['lookahead'])

    # ---- what a route is ----------------------------------------------------------------------------------------------------------
    lanes = property(lambda self: self._t['lanes'])
    n = property(lambda self: self._t['n'])
    start_arc = property(lambda self: self._t['start_arc'])
    end_arc = property(lambda self: self._t['end_arc'])
    offsets = property(lambda self: self._t['offsets'])
    length = property(lambda self: self._t['length'])
    cursor = property(lambda self: self._t['cursor'])
    scene_ids = property(lambda self: self._t['scene_ids'])
    requested_length = property(lambda self: self._t['distance'])
    # of routes to a destination (`RouteGoal.to`, `resample_to`); objects that never had destinations do not have them
    destination_lanes = property(lambda self: self._t['dest_lane'])
    destination_arcs = property(lambda self: self._t['dest_arc'])

    @property
    def rest(self) -> Tensor:
        """(B, A) float64: what is left to the destination from the END of the route: 0 for a route that reaches it, positive for one cut at 16
        lanelets, inf where the destination cannot be reached or the row has no route to one"""
        return self._t['rest']

    @property
    def truncated(self) -> Tensor:
        """(B, A) bool: the route was cut at 16 lanelets short of its destination (`rest` > 0 and finite)"""
        rest = self._t['rest']
        return (rest > 0) & torch.isfinite(rest)

    @property
    def completed(self) -> Tensor:
        """(B, A) bool, sticky: the agent has been within `goal_tolerance` of its route's end since the route was dealt"""
        return self._t['completed'].view(torch.bool)

    @property
    def valid(self) -> Tensor:
        """(B, A) bool: the agent has a route"""
        return self._t['n'] > 0

    def points(self, arcs: Tensor) -> Tensor:
        """World-frame points at route arcs: arcs (B, A, Q), or (Q,) for the same arcs on every route -> (B, A, Q, 2) float32.  Arcs are clamped to
        [0, length]; rows without a route give [0, 0]."""
        from torchdrivesim_amd import _ops
        if not arcs.is_cuda:
            raise RuntimeError(f'arcs: route goals run on an MI355X; got a {arcs.device} tensor (no CPU fallback)')
        B, A = self._t['n'].shape
        if arcs.dim() == 1:
            arcs = arcs.view(1, 1, -1).expand(B, A, -1)
        if B * A == 0:
            return torch.zeros((B, A, arcs.shape[-1], 2), dtype=torch.float32, device=arcs.device)
        return _ops.route_points(self._lane_table_set(), self._t, arcs)

    def waypoint_goal(self, spacing: float = 4.0) -> WaypointGoal:
        """The routes as a `WaypointGoal` the renderer draws as goal discs: N = floor(longest route / spacing) + 1 collections of ONE point each,
        point i at route arc i * spacing (B x A x N x 1 x 2); its mask is True where i * spacing <= the route's length and the row has a route."""
        if not spacing > 0:
            raise ValueError(f'spacing must be > 0, got {spacing}')
        length = self._t['length']
        longest = float(length.max()) if length.numel() > 0 else 0.0
        arcs = torch.arange(int(longest / spacing) + 1, dtype=torch.float64, device=length.device) * float(spacing)
        mask = (arcs.view(1, 1, -1) <= length.unsqueeze(-1)) & self.valid.unsqueeze(-1)
        return WaypointGoal(self.points(arcs).unsqueeze(3), mask.unsqueeze(3))

    # ---- batch plumbing ---------------------------------------------------------------------------------------------------------
    def _map(self, f):
        # the kernels update these in place: dense tensors of their own types, owned by this object
        self._t = {k: f(v).contiguous() for k, v in self._t.items()}
        self._lanes = None
        self._lane_table_set()
        return self

    def copy(self):
        return self.__class__(self.lanelet_maps, {k: v.clone() for k, v in self._t.items()}, seed=self.seed, tolerance=self.tolerance,
                              goal_tolerance=self.goal_tolerance, off_route_distance=self.off_route_distance, lookahead=self.lookahead,
                              spacing=self.spacing, differentiable=self.differentiable)

    def _to_device(self, device):
        return self._map(lambda x: x.to(device))

    to = _ClassOrInstance(_to_destination, _to_device)

    def extend(self, n: int, in_place: bool = True):
        from torchdrivesim_amd.lanelet2 import LaneletMap
        me = self if in_place else self.copy()
        if not isinstance(me.lanelet_maps, LaneletMap):
            me.lanelet_maps = [m for m in me.lanelet_maps for _ in range(n)]
        return me._map(lambda x: x.unsqueeze(1).expand((x.shape[0], n) + x.shape[1:]).reshape((n * x.shape[0],) + x.shape[1:]))

    def select_batch_elements(self, idx, in_place: bool = True):
        from torchdrivesim_amd.lanelet2 import LaneletMap
        me = self if in_place else self.copy()
        if not isinstance(me.lanelet_maps, LaneletMap):
            me.lanelet_maps = [me.lanelet_maps[int(i)] for i in idx]
        return me._map(lambda x: x[idx])
