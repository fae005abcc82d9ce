"""Numpy restatement of the two definitions of include/tdship.h "K7" (DESIGN.md 5.5h), which the kernels of csrc/lights.hip must equal bit for bit:
the light programmes over their TABLES -- float64 + - and comparisons, TrafficLightStateMachine.tick operation for operation -- and the stop-line
selection in binary32, every operation rounded once (numpy float32 arithmetic does not contract)."""
import numpy as np

import spawn_model as sm

MAX_SKIPS, MAX_MACHINES, MAX_PHASES, MAX_LIGHTS, MAX_K = 1024, 256, 64, 1024, 32
ALLOWED = ('red', 'yellow', 'green')
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- programmes
def tables(programmes, light_ids, allowed=ALLOWED):
    """programmes: the controller's JSON form, a list of machines, each a list of {"actor_states": {id: colour}, "state", "duration",
    "next_state"} -> dict(duration MxP float64, next_phase MxP int32, n_phases M int32, sequence_number MxP int32, colour MxPxN uint8)"""
    M, N, P = len(programmes), len(light_ids), max(len(m) for m in programmes)
    t = dict(duration=np.ones((M, P)), next_phase=np.tile(np.arange(P, dtype=np.int32), (M, 1)), n_phases=np.array([len(m) for m in programmes], np.int32),
             sequence_number=np.zeros((M, P), np.int32), colour=np.full((M, P, N), 255, np.uint8))
    for m, machine in enumerate(programmes):
        for p, phase in enumerate(machine):
            t['duration'][m, p], t['next_phase'][m, p], t['sequence_number'][m, p] = float(phase['duration']), int(phase['next_state']), int(phase['state'])
            for n, i in enumerate(light_ids):
                if str(i) in phase['actor_states']:
                    t['colour'][m, p, n] = allowed.index(phase['actor_states'][str(i)])
    return t


def tick_machine(duration, next_phase, p, r, dt):
    """one machine: (phase, remaining) after dt, as the definition states it"""
    left = r - dt
    if left > 0:
        return p, left
    nxt, span = p, 0.0
    for _ in range(MAX_SKIPS):
        nxt = int(next_phase[p])
        span = float(duration[nxt])
        if left == 0:
            return nxt, span
        left += span
        if left > 0:
            return nxt, (left if left <= span else span)
        p = nxt
    return nxt, span


def reset_phase(seed, scene_id, m, n):
    """(r0 * n) >> 32 with r0 the first word of Philox4x32-10, key (seed low ^ 'LIGH', seed high ^ 'TSTR'), counter (scene id low, high, m, 0)"""
    seed, scene_id = int(seed) & (2 ** 64 - 1), int(scene_id) & (2 ** 64 - 1)
    r0 = sm.philox4x32_10((scene_id & 0xFFFFFFFF, scene_id >> 32, m, 0), ((seed & 0xFFFFFFFF) ^ 0x4C494748, (seed >> 32) ^ 0x54535452))[0]
    return (int(r0) * int(n)) >> 32


class Lights:
    """the state of B scenes over one set of tables: phase BxM int32, remaining BxM float64, state BxN int64, time_to_change BxN float32"""

    def __init__(self, t, B):
        self.t = t
        M, N = t['n_phases'].shape[0], t['colour'].shape[2]
        self.phase = np.zeros((B, M), np.int32)
        self.remaining = np.zeros((B, M), np.float64)
        self.state = np.zeros((B, N), np.int64)
        self.time_to_change = np.zeros((B, N), F32)

    def _scenes(self, mask):
        return [b for b in range(self.phase.shape[0]) if mask is None or mask[b]]

    def refresh(self, mask=None):
        """step 2: every light takes the colour of the LAST machine whose current phase names it; others keep what they had"""
        for b in self._scenes(mask):
            for m in range(self.phase.shape[1]):
                c = self.t['colour'][m, self.phase[b, m]]
                named = c != 255
                self.state[b, named] = c[named]
                self.time_to_change[b, named] = F32(self.remaining[b, m])

    def tick(self, dt, mask=None):
        for b in self._scenes(mask):
            for m in range(self.phase.shape[1]):
                self.phase[b, m], self.remaining[b, m] = tick_machine(self.t['duration'][m], self.t['next_phase'][m], int(self.phase[b, m]),
                                                                      float(self.remaining[b, m]), float(dt))
        self.refresh(mask)

    def set_to(self, rows, scenes=None):
        """rows: [(phase index, seconds)] for the first len(rows) machines, clamped as the host's set_to"""
        for b in (range(self.phase.shape[0]) if scenes is None else scenes):
            for m, (p, time) in enumerate(rows):
                p = min(max(int(p), 0), int(self.t['n_phases'][m]) - 1)
                span = self.t['duration'][m, p]
                self.phase[b, m], self.remaining[b, m] = p, (time if time <= span else span)
        self.refresh()

    def reset(self, seed, scene_ids, mask=None):
        for b in self._scenes(mask):
            for m in range(self.phase.shape[1]):
                p = reset_phase(seed, scene_ids[b], m, self.t['n_phases'][m])
                self.phase[b, m], self.remaining[b, m] = p, self.t['duration'][m, p]
        self.refresh(mask)

    @property
    def state_per_machine(self):
        return np.take_along_axis(np.broadcast_to(self.t['sequence_number'], self.phase.shape + self.t['sequence_number'].shape[1:]),
                                  self.phase[..., None].astype(np.int64), 2)[..., 0]


def random_programmes(seed, M, P, N, exact=False, first_id=100):
    """M machines of 1 .. P phases (machine 0 has exactly P) over N lights: machine m names in EVERY phase the lights n with n % M == m, and in some
    phases any other light (ids shared between machines: the later machine wins).  Durations are multiples of 1/8 s from 0.5 s (binary-exact, so that ticks of
    1/8 s end phases exactly: the `left == 0` branch) with exact=True, arbitrary doubles of 0.5 .. 9 s else; next_state is any phase of the machine
    -> (programmes in the JSON form, light ids)"""
    g = np.random.default_rng(seed)
    ids = [first_id + n for n in range(N)]
    programmes = []
    for m in range(M):
        n_ph = P if m == 0 else int(g.integers(1, P + 1))
        order = g.permutation(n_ph)
        machine = []
        for p in range(n_ph):
            own = {str(ids[n]): ALLOWED[int(g.integers(3))] for n in range(N) if n % M == m}
            extra = {str(ids[n]): ALLOWED[int(g.integers(3))] for n in range(N) if n % M != m and g.random() < 0.3}
            duration = float(g.integers(4, 41)) / 8.0 if exact else float(g.uniform(0.5, 9.0))
            machine.append(dict(actor_states={**own, **extra}, state=str(int(order[p])), duration=duration, next_state=str(int(g.integers(n_ph)))))
        programmes.append(machine)
    return programmes, ids


# ---------------------------------------------------------------------------------------------------------------- stop lines
def stop_lines(agent_xy, agent_sc, agent_present, lines, line_sc, mask, state, time_to_change, k, max_distance, ahead_only=True, min_cos=None):
    """agent_xy (B,A,2), agent_sc (B,A,2), agent_present (B,A), lines (B,N,5), line_sc (B,N,2), mask (B,N), state (B,N), time_to_change None or
    (B,N) -> features (B,A,k,8) float32, index (B,A,k) int32, state (B,A,k) int32"""
    agent_xy, agent_sc, lines, line_sc = (np.asarray(v, F32) for v in (agent_xy, agent_sc, lines, line_sc))
    agent_present, mask = np.asarray(agent_present).astype(bool), np.asarray(mask).astype(bool)
    B, A = agent_xy.shape[:2]
    N, K = lines.shape[1], int(k)
    assert 1 <= K <= MAX_K and N <= MAX_LIGHTS and not (F32(max_distance) < 0) and not np.isnan(max_distance)
    min_cos = F32(-np.inf) if min_cos is None else F32(min_cos)
    ttc = np.zeros((B, N), F32) if time_to_change is None else np.asarray(time_to_change, F32)
    features = np.zeros((B, A, K, 8), F32)
    index = np.full((B, A, K), -1, np.int32)
    slot_state = np.full((B, A, K), -1, np.int32)
    who_all = np.arange(N)
    with np.errstate(over='ignore', invalid='ignore'):
        r2 = F32(max_distance) * F32(max_distance)
        for b in range(B):
            sl, cl = line_sc[b, :, 0], line_sc[b, :, 1]
            for a in range(A):
                if not agent_present[b, a]:
                    continue
                s, c = agent_sc[b, a]
                dx, dy = lines[b, :, 0] - agent_xy[b, a, 0], lines[b, :, 1] - agent_xy[b, a, 1]
                d2 = dx * dx + dy * dy
                x, y = dx * c + dy * s, dy * c - dx * s
                sin_rel, cos_rel = sl * c - cl * s, cl * c + sl * s
                cand = mask[b] & (d2 <= r2) & (cos_rel >= min_cos)              # (a NaN fails every comparison)
                if ahead_only:
                    cand &= x >= 0
                who = who_all[cand]
                who = who[np.lexsort((who, d2[cand]))][:K]                      # by d2, equal d2 by the lower index
                n = len(who)
                features[b, a, :n] = np.stack([x[who], y[who], sin_rel[who], cos_rel[who], lines[b, who, 2], lines[b, who, 3], ttc[b, who],
                                               np.sqrt(d2[who])], -1)
                index[b, a, :n] = who
                slot_state[b, a, :n] = np.asarray(state)[b, who]
    return features, index, slot_state


def heading_sc(psi):
    return np.stack([np.sin(psi.astype(np.float64)), np.cos(psi.astype(np.float64))], -1).astype(F32)


DEFINITION_MAX_DISTANCE = 10.0


def definition_cases():
    """B = 2, A = 3, N = 6, to be asked for K = 4 within DEFINITION_MAX_DISTANCE; headings are exact [sin, cos] pairs.
    scene 0: observer 0 at the origin looking along +x, observer 1 at the origin looking along -x, observer 2 absent.  Lines 0 and 1 mirrored across
             the x axis (bit-equal d2 = 25: 0 comes first), line 1 turned by pi (cos_rel = -1 for observer 0); line 2 at d2 = 100 = r2 exactly (in);
             line 3 a float32 step beyond (out); line 4 three metres BEHIND observer 0 (ahead of observer 1); line 5, the nearest of all, is masked.
    scene 1: observer 0 stands on line 0 (d2 = 0, x = 0: still "ahead"); observer 1 has a NaN pose (an empty row); observer 2 one metre before
             line 0; line 1 has a NaN pose (never a candidate); line 2 is out of range; lines 3 .. 5 are masked."""
    agent_xy = np.zeros((2, 3, 2), F32)
    agent_sc = np.zeros((2, 3, 2), F32)
    agent_sc[..., 1] = 1.0
    agent_sc[0, 1] = [0.0, -1.0]
    agent_present = np.ones((2, 3), bool)
    agent_present[0, 2] = False
    agent_xy[1] = [[1, 1], [np.nan, 1], [0, 1]]
    lines = np.zeros((2, 6, 5), F32)
    lines[..., 2], lines[..., 3] = [0.5, 0.6, 0.7, 0.8, 0.9, 1.0], [3.0, 3.5, 4.0, 4.5, 5.0, 5.5]
    lines[0, :, :2] = [[3, 4], [3, -4], [6, 8], [np.nextafter(F32(6), F32(7)), 8], [-3, 0], [1, 0]]
    lines[1, :, :2] = [[1, 1], [np.nan, 1], [100, 100], [1, 1], [1, 2], [2, 1]]
    line_sc = np.zeros((2, 6, 2), F32)
    line_sc[..., 1] = 1.0
    line_sc[0, 1] = [0.0, -1.0]
    mask = np.ones((2, 6), bool)
    mask[0, 5] = False
    mask[1, 3:] = False
    state = np.array([[0, 1, 2, 0, 1, 2], [2, 1, 0, 2, 1, 0]], np.int64)
    time_to_change = np.array([[1.5, 2.5, 3.5, 4.5, 5.5, 6.5], [0.25, 0.5, 0.75, 1.0, 1.25, 1.5]], F32)
    d2 = lines[0, 3, 0] * lines[0, 3, 0] + lines[0, 3, 1] * lines[0, 3, 1]
    assert d2 == np.nextafter(F32(100), F32(200)) and F32(DEFINITION_MAX_DISTANCE) * F32(DEFINITION_MAX_DISTANCE) == F32(100)
    return dict(agent_xy=agent_xy, agent_sc=agent_sc, agent_present=agent_present, lines=lines, line_sc=line_sc, mask=mask, state=state,
                time_to_change=time_to_change)


E4 = [-1, -1, -1, -1]
#: the index tensor of definition_cases() at K = 4, by hand from the definition, per (ahead_only, min_cos)
DEFINITION_INDEX = {
    (True, None): [[[0, 1, 2, -1], [4, -1, -1, -1], E4], [[0, -1, -1, -1], E4, [0, -1, -1, -1]]],
    (False, None): [[[4, 0, 1, 2], [4, 0, 1, 2], E4], [[0, -1, -1, -1], E4, [0, -1, -1, -1]]],
    (True, 0.5): [[[0, 2, -1, -1], E4, E4], [[0, -1, -1, -1], E4, [0, -1, -1, -1]]],
}


def random_scenes(seed, B, A, N, side=120.0, duplicates=0.1, absent=0.1):
    """float32 poses in a square of `side` metres; a share of the lines lies exactly on another one (bit-equal d2 for every observer), a share of
    lines and observers is absent; one observer per scene stands exactly on a line -> the arguments of stop_lines as a dict"""
    g = np.random.default_rng(seed)
    lines = np.concatenate([g.uniform(0, side, (B, N, 2)), g.uniform(0.3, 1.0, (B, N, 1)), g.uniform(3.0, 7.0, (B, N, 1)), g.uniform(-np.pi, np.pi, (B, N, 1))],
                           -1).astype(F32)
    for b in range(B):
        for n in np.nonzero(g.random(N) < duplicates)[0]:
            lines[b, n, :2] = lines[b, g.integers(N), :2]
    agent_xy = g.uniform(0, side, (B, A, 2)).astype(F32)
    agent_xy[:, 0] = lines[:, N // 2, :2]
    return dict(agent_xy=agent_xy, agent_sc=heading_sc(g.uniform(-np.pi, np.pi, (B, A)).astype(F32)), agent_present=g.random((B, A)) >= absent, lines=lines,
                line_sc=heading_sc(lines[..., 4]), mask=g.random((B, N)) >= absent, state=g.integers(0, 3, (B, N)).astype(np.int64),
                time_to_change=g.uniform(0, 30, (B, N)).astype(F32))
