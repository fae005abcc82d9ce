"""
Traffic controls: static rectangular stop lines with a discrete state per element (torchdrivesim/traffic_controls.py).
Same class surface as the reference (`BaseTrafficControl`, `TrafficLightControl`, `StopSignControl`, `YieldControl`); the one
computation on the hot path -- which agents overlap a red light's stop line -- runs on K2a's box-intersection kernel.
"""
from typing import List, Optional

import torch
from torch import Tensor

from torchdrivesim_amd import _ops


def _rear_boxes(boxes: Tensor, rear_factor: float) -> Tensor:
    """The rear `rear_factor` part of every box as a box of its own: same heading and width, length * rear_factor, centre
    moved back by length * (1 - rear_factor) / 2 (box2corners_with_rear_factor, _iou_utils.py:302-341).  boxes (...,5) [x,y,l,w,psi]."""
    x, y, l, w, psi = boxes.unbind(-1)
    back = (l * (1 - rear_factor)) / 2
    return torch.stack([x - back * torch.cos(psi), y - back * torch.sin(psi), l * rear_factor, w, psi], dim=-1)


class BaseTrafficControl:
    """
    pos: BxNx5 stop lines [x, y, length (thickness), width, orientation]; allowed_states: names of the discrete states;
    replay_states: BxNxT indices into allowed_states replayed by `step` while t < T; mask: BxN, False for padding
    (traffic_controls.py:12-156).
    """

    def __init__(self, pos: Tensor, allowed_states: Optional[List[str]] = None, replay_states: Optional[Tensor] = None,
                 mask: Optional[Tensor] = None):
        self.pos = pos
        self.allowed_states = list(allowed_states) if allowed_states is not None else self._default_allowed_states()
        self.replay_states = replay_states if replay_states is not None else \
            torch.zeros(pos.shape[:2] + (0,), dtype=torch.long, device=pos.device)
        self.mask = mask if mask is not None else torch.ones(pos.shape[:2], dtype=torch.bool, device=pos.device)
        self.state = self.replay_states[..., 0] if self.total_replay_time > 0 else \
            torch.zeros(pos.shape[:2], dtype=torch.long, device=pos.device)

    @classmethod
    def _default_allowed_states(cls) -> List[str]:
        return ['none']

    @property
    def total_replay_time(self) -> int:
        return self.replay_states.shape[-1]

    @property
    def corners(self) -> Tensor:
        """BxNx4x2 corners of the stop lines; padding elements are parked far away (traffic_controls.py:31-33)"""
        c = _box_corners(self.pos)
        m = self.mask.to(c.dtype)[..., None, None]
        return c * m + (1 - m) * -1000

    def _tensors(self):
        return ('pos', 'replay_states', 'mask', 'state')

    def copy(self):
        other = self.__class__(pos=self.pos.clone(), allowed_states=list(self.allowed_states), replay_states=self.replay_states.clone(),
                               mask=self.mask.clone())
        other.state = self.state.clone()
        return other

    def to(self, device):
        for n in self._tensors():
            setattr(self, n, getattr(self, n).to(device))
        return self

    def extend(self, n: int, in_place: bool = True):
        """repeat every batch element n times (B -> B*n, element-major), as the Simulator does for n cameras"""
        tgt = self if in_place else self.copy()
        for name in tgt._tensors():
            t = getattr(tgt, name)
            setattr(tgt, name, t.unsqueeze(1).expand((t.shape[0], n) + t.shape[1:]).reshape((n * t.shape[0],) + t.shape[1:]))
        return tgt

    def select_batch_elements(self, idx: Tensor, in_place: bool = True):
        tgt = self if in_place else self.copy()
        for name in tgt._tensors():
            setattr(tgt, name, getattr(tgt, name)[idx])
        return tgt

    def set_state(self, state: Tensor) -> None:
        self.state = state

    def compute_state(self, time: int) -> Tensor:
        """state at `time` beyond the replayed history: by default the current state is kept"""
        return self.state

    def step(self, time: int) -> None:
        self.set_state(self.replay_states[..., time] if time < self.total_replay_time else self.compute_state(time))

    def compute_violation(self, agent_state: Tensor) -> Tensor:
        """agent_state BxAx5 [x,y,length,width,orientation] -> BxA bool; the base class reports none"""
        return torch.zeros(agent_state.shape[:2], dtype=torch.bool, device=agent_state.device)


def _box_corners(pos: Tensor) -> Tensor:
    if pos.is_cuda:
        return _ops.box2corners(pos)
    # host-side plumbing (construction on the CPU before .to(device)): the same formula in torch (_iou_utils.py:270-299)
    x4 = torch.tensor([0.5, -0.5, -0.5, 0.5], dtype=pos.dtype) * pos[..., 2:3]
    y4 = torch.tensor([0.5, 0.5, -0.5, -0.5], dtype=pos.dtype) * pos[..., 3:4]
    s, c = torch.sin(pos[..., 4:5]), torch.cos(pos[..., 4:5])
    return torch.stack([x4 * c - y4 * s + pos[..., 0:1], x4 * s + y4 * c + pos[..., 1:2]], dim=-1)


class TrafficLightControl(BaseTrafficControl):
    """States ['red', 'yellow', 'green'].  An agent violates a light when the light is red and the rear tenth of the agent's box
    overlaps the stop line, i.e. it has driven (almost) completely over it (traffic_controls.py:159-194)."""
    violation_rear_factor = 0.1

    @classmethod
    def _default_allowed_states(cls) -> List[str]:
        return ['red', 'yellow', 'green']

    def compute_violation(self, agent_state: Tensor) -> Tensor:
        B, A = agent_state.shape[:2]
        N = self.pos.shape[1]
        if B == 0 or A == 0 or N == 0:
            return torch.zeros(B, A, dtype=torch.bool, device=agent_state.device)
        rear = _rear_boxes(agent_state, self.violation_rear_factor)                       # B x A x 5
        # padding stop lines are parked at (-1000, -1000) like the reference's corners (traffic_controls.py:31-33)
        key = (self.pos.data_ptr(), self.pos._version, tuple(self.pos.shape), self.mask.data_ptr(), self.mask._version, str(rear.device), A)
        cached = getattr(self, '_lines_cache', None)
        if cached is None or cached[0] != key:              # the stop lines do not move: their (B, A*N, 5) operand is built once
            m = self.mask.to(self.pos.dtype)[..., None]
            park = torch.tensor([-1000.0, -1000.0, 0.0, 0.0, 0.0], dtype=self.pos.dtype).to(self.pos.device)
            lines = (self.pos * m + (1 - m) * park).to(rear.device)
            cached = (key, lines[:, None, :, :].expand(B, A, N, 5).reshape(B, A * N, 5).contiguous())
            self._lines_cache = cached
        b1 = rear[:, :, None, :].expand(B, A, N, 5).reshape(B, A * N, 5)
        b2 = cached[1]
        overlap = _ops.pairwise_overlap(b1.contiguous(), b2.contiguous(), metric='iou').reshape(B, A, N) > 0
        red = (self.state.to(overlap.device) == self.allowed_states.index('red'))[:, None, :]
        return (overlap & red).any(dim=-1)


class YieldControl(BaseTrafficControl):
    """Yield sign: cross traffic has priority.  No violations are computed."""


class StopSignControl(BaseTrafficControl):
    """Stop sign.  No violations are computed."""


def light_programme_tables(controller, light_ids, allowed_states, dt=0.1):
    """The device tables of `ProgrammedTrafficLightControl` from a host `traffic_lights.TrafficLightController`, as CPU tensors: a dict of
    duration MxP float64, next_phase MxP int32 (the LIST POSITION `TrafficLightStateMachine.tick` indexes its phases with), n_phases M int32,
    sequence_number MxP int32 (what `state_per_machine` reports) and colour MxPxN uint8 (index into `allowed_states` of light `light_ids[n]`,
    255 where the phase does not name it).  Shorter machines are padded with phases of one second that lead to themselves and name nothing.
    ValueError for what the kernel must never meet: see the class."""
    import math
    from torchdrivesim_amd import _native as nat
    machines = [fsm.states for fsm in controller.traffic_fsms]
    M, N = len(machines), len(light_ids)
    if M == 0 or any(len(phases) == 0 for phases in machines):
        raise ValueError('traffic lights: a controller needs at least one machine, and every machine a phase')
    P = max(len(phases) for phases in machines)
    duration = torch.ones((M, P), dtype=torch.float64)
    next_phase = torch.arange(P, dtype=torch.int32).repeat(M, 1)
    sequence_number = torch.zeros((M, P), dtype=torch.int32)
    colour = torch.full((M, P, N), 255, dtype=torch.uint8)
    column = {str(i): n for n, i in enumerate(light_ids)}
    if len(column) != N:
        raise ValueError('traffic lights: light_ids repeats an id')
    always = torch.zeros(N, dtype=torch.bool)
    for m, phases in enumerate(machines):
        for p, phase in enumerate(phases):
            d, nxt = float(phase.duration), int(phase.next_state)
            if not (math.isfinite(d) and d > 0):
                raise ValueError(f'traffic lights: machine {m}, phase {p}: the duration must be finite and > 0 (got {phase.duration})')
            if not 0 <= nxt < len(phases):
                raise ValueError(f'traffic lights: machine {m}, phase {p}: next_state {nxt} is outside the machine\'s {len(phases)} phases')
            duration[m, p], next_phase[m, p], sequence_number[m, p] = d, nxt, int(phase.sequence_number)
            for actor, state in phase.actor_states.items():
                if actor in column:
                    if state.name not in allowed_states:
                        raise ValueError(f'traffic lights: machine {m}, phase {p}: light {actor} is {state.name!r}, which is none of {allowed_states}')
                    colour[m, p, column[actor]] = allowed_states.index(state.name)
        always |= (colour[m, :len(phases)] != 255).all(dim=0)
    if not bool(always.all()):
        missing = [light_ids[n] for n in torch.nonzero(~always).flatten().tolist()]
        raise ValueError(f'traffic lights: no machine names light(s) {missing} in every one of its phases: they would have no colour at times')
    shortest = min(float(phase.duration) for phases in machines for phase in phases)
    if not (math.isfinite(dt) and 0 <= dt <= nat.LIGHTS_MAX_SKIPS * shortest):
        raise ValueError(f'traffic lights: dt must be finite, not negative and at most {nat.LIGHTS_MAX_SKIPS} x the shortest phase ({shortest} s), got {dt}')
    return dict(duration=duration, next_phase=next_phase, n_phases=torch.tensor([len(phases) for phases in machines], dtype=torch.int32),
                sequence_number=sequence_number, colour=colour)


class ProgrammedTrafficLightControl(TrafficLightControl):
    """Traffic lights whose programmes run ON THE DEVICE, a clock per scene (csrc/lights.hip; the definition is in include/tdship.h "K7").
    Built from a host `traffic_lights.TrafficLightController`, whose phases become tables shared by the batch; `light_ids[n]` is the id of stop
    line n of `pos` (BxNx5).  Per scene it owns `phase` BxM int32 (list position), `remaining` BxM float64, `state` BxN int64 -- the attribute
    every consumer of a TrafficLightControl reads, here written IN PLACE and never replaced --, `time_to_change` BxN float32 and `scene_ids`.
    `step` (and so `Simulator.step`) advances every machine of every scene by `dt` in one launch; the arithmetic is
    `TrafficLightStateMachine.tick`'s in float64, bit for bit.  `reset` deals the masked scenes a random phase that depends on (seed, scene id)
    only.  ValueError at construction for a duration that is not finite and > 0, a next_state outside its machine, a colour outside
    `allowed_states`, a light that no machine names in every phase, and a dt that is negative, non-finite or longer than 1024 shortest phases."""

    _TABLES = ('duration', 'next_phase', 'n_phases', 'sequence_number', 'colour')

    def __init__(self, pos: Tensor, controller, light_ids, dt: float = 0.1, seed: int = 0, scene_ids: Optional[Tensor] = None,
                 mask: Optional[Tensor] = None):
        super().__init__(pos, mask=mask)
        light_ids = [int(i) for i in light_ids]
        if pos.dim() != 3 or pos.shape[1] != len(light_ids):
            raise ValueError(f'traffic lights: pos {tuple(pos.shape)} for {len(light_ids)} light ids')
        tables = light_programme_tables(controller, light_ids, self.allowed_states, dt)
        if not pos.is_cuda:
            raise RuntimeError(f'ProgrammedTrafficLightControl runs on an MI355X; pos is on {pos.device} (no CPU fallback)')
        dev, B, M = pos.device, pos.shape[0], tables['n_phases'].shape[0]
        self.tables = {k: v.to(dev) for k, v in tables.items()}
        self.light_ids, self.dt, self.seed = light_ids, float(dt), int(seed)
        self.phase = torch.zeros((B, M), dtype=torch.int32, device=dev)
        self.remaining = torch.zeros((B, M), dtype=torch.float64, device=dev)
        self.time_to_change = torch.zeros((B, len(light_ids)), dtype=torch.float32, device=dev)
        self.scene_ids = torch.arange(B, dtype=torch.int64, device=dev)
        self.reset(scene_ids=scene_ids)

    def _tensors(self):
        return super()._tensors() + ('phase', 'remaining', 'time_to_change', 'scene_ids')

    def _kernel_tables(self):
        t = self.tables
        return t['duration'], t['next_phase'], t['n_phases'], t['colour']

    def _dense(self):
        for n in ('state', 'phase', 'remaining', 'time_to_change', 'scene_ids'):
            setattr(self, n, getattr(self, n).contiguous())
        return self

    def copy(self):
        other = object.__new__(self.__class__)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ('_lines_cache', '_line_sc_cache')})
        other.allowed_states, other.light_ids = list(self.allowed_states), list(self.light_ids)
        for n in self._tensors():
            setattr(other, n, getattr(self, n).clone())
        return other

    def to(self, device):
        super().to(device)
        self.tables = {k: v.to(device) for k, v in self.tables.items()}
        return self

    def extend(self, n: int, in_place: bool = True):
        return super().extend(n, in_place)._dense()

    def select_batch_elements(self, idx, in_place: bool = True):
        return super().select_batch_elements(idx, in_place)._dense()

    def set_state(self, state: Tensor) -> None:
        """the colours, copied INTO `state` (the programme overwrites them at its next tick)"""
        if state is not self.state:
            self.state.copy_(state)

    def tick(self, dt: float) -> Tensor:
        """every machine of every scene advanced by `dt` seconds, through as many phases as that spans: one launch"""
        _ops.lights_step(self._kernel_tables(), self.phase, self.remaining, self.state, self.time_to_change, dt)
        return self.state

    def compute_state(self, time: int) -> Tensor:
        return self.tick(self.dt)

    def set_to(self, light_states) -> None:
        """Jump to (phase index, seconds remaining) per machine: a B x m x 2 tensor, or the host's list form [[index, seconds], ...] for the first m
        machines, applied to every scene.  Clamped as the host's `set_to`: the index into the machine, the time to at most the phase's duration.
        `state` and `time_to_change` follow; no time passes."""
        t = torch.as_tensor(light_states, dtype=torch.float64).to(self.phase.device)
        if t.dim() == 2:
            t = t.unsqueeze(0).expand(self.phase.shape[0], -1, -1)
        m = t.shape[1]
        if t.dim() != 3 or t.shape[0] != self.phase.shape[0] or m > self.phase.shape[1] or t.shape[2] != 2:
            raise ValueError(f'set_to: expected ({self.phase.shape[0]}, m <= {self.phase.shape[1]}, 2), got {tuple(t.shape)}')
        index = torch.minimum(t[..., 0].to(torch.int64).clamp(min=0), self.tables['n_phases'][:m].to(torch.int64) - 1)
        span = torch.gather(self.tables['duration'][:m].expand(t.shape[0], -1, -1), 2, index.unsqueeze(-1)).squeeze(-1)
        self.phase[:, :m] = index.to(torch.int32)
        self.remaining[:, :m] = torch.where(t[..., 1] <= span, t[..., 1], span)
        _ops.lights_step(self._kernel_tables(), self.phase, self.remaining, self.state, self.time_to_change, 0.0, advance=False)

    def reset(self, mask: Optional[Tensor] = None, scene_ids: Optional[Tensor] = None) -> None:
        """Every machine of the scenes where `mask` (B bool) is set -- all scenes without one -- to the beginning of a random phase, in place: two
        launches, no allocation, no synchronisation.  The phase depends on (seed, scene id, machine) only, so a scene's lights are the same in
        any batch or shard that holds it; new `scene_ids` (B int64) are stored first."""
        if scene_ids is not None:
            self.scene_ids.copy_(scene_ids)
        _ops.lights_reset(self._kernel_tables(), self.phase, self.remaining, self.scene_ids, self.seed, mask=mask)
        _ops.lights_step(self._kernel_tables(), self.phase, self.remaining, self.state, self.time_to_change, 0.0, advance=False, mask=mask)

    @property
    def state_per_machine(self) -> Tensor:
        """BxM: the `sequence_number` of every machine's current phase (TrafficLightController.state_per_machine)"""
        seq = self.tables['sequence_number'].expand(self.phase.shape[0], -1, -1)
        return torch.gather(seq, 2, self.phase.to(torch.int64).unsqueeze(-1)).squeeze(-1)

    @property
    def time_remaining(self) -> Tensor:
        """BxM float64: seconds left in every machine's current phase"""
        return self.remaining
