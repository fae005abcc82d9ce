"""
Shapes and input sets of the occlusion-mask tests (tds_occlusion_mask_f32, csrc/collision.hip: one wave per (scene, ego), lanes = targets in
chunks of 64, loop over occluders), shared by tests/test_occlusion_cases.py (CPU: does each set contain what it is there for, judged on the
oracle alone?) and tests/test_gpu_occlusion.py.

state (B, E, 4) [x, y, psi, v], size (B, E, 2) [length, width], present (B, E); the first A entities are the egos.
"""
import numpy as np

# (B, A, E)
SHAPES = [
    (1, 1, 1),                          # nobody to hide behind
    (3, 5, 63), (3, 5, 64), (2, 6, 65),  # around one chunk of 64 targets: a last chunk of 63, 64 and 1 lanes
    (2, 3, 130),                        # three chunks, the last one of 2 lanes
    (1, 70, 70),                        # egos beyond the first chunk (the `o != a` exclusion with a >= 64)
    (5, 1, 200),                        # B * A = 5 waves: the second block of 4 waves holds one
]
SETS = ('random', 'in_line', 'coincident', 'tangent', 'zero_width', 'absent_occluder', 'nan_row')
MIN_E = 6                               # the hand-placed sets need a few entities


def cases():
    return [(B, A, E, s) for (B, A, E) in SHAPES for s in SETS if s == 'random' or E >= MIN_E]


def _random(gen, B, E):
    """a 60 m box; widths shrink with the head count so that neither everybody nor nobody is hidden"""
    xy = gen.uniform(-30.0, 30.0, (B, E, 2))
    state = np.concatenate([xy, gen.uniform(-np.pi, np.pi, (B, E, 1)), gen.uniform(0.0, 10.0, (B, E, 1))], -1)
    w = gen.uniform(0.8, 2.4, (B, E)) * min(1.0, 24.0 / E)
    size = np.stack([gen.uniform(3.0, 6.0, (B, E)), w], -1)
    present = gen.uniform(size=(B, E)) < 0.85
    return state, size, present


def make(B, A, E, name):
    """(state, size, present, marks): marks is a list of (b, a, e, hidden) entries that the set is built to produce"""
    gen = np.random.default_rng([B, A, E, SETS.index(name)])
    state, size, present = _random(gen, B, E)
    marks = []
    if name == 'random' or E < MIN_E:
        return state.astype(np.float32), size.astype(np.float32), present, marks
    far = np.array([500.0, 500.0])          # hand-placed groups go far away from the random crowd, one group per scene
    for b in range(B):
        ego, tgt, occ = 0, E - 1, E // 2      # the target and the occluder lie in the last and in a middle chunk
        base = far + 100.0 * b
        if name == 'in_line':
            # exactly collinear: the occluder halfway, the target at twice the offset (binary fractions of the offset: no rounding)
            off = np.array([gen.integers(4, 12) * 2.0, gen.integers(-6, 6) * 2.0])
            state[b, ego, :2], state[b, occ, :2], state[b, tgt, :2] = base, base + off / 2, base + off
            present[b, occ] = True
            marks += [(b, ego, tgt, True), (b, ego, occ, False)]
            if A > 1:                         # seen from the side, nothing is in the way
                state[b, 1, :2] = base + np.array([-off[1], off[0]])
                marks += [(b, 1, tgt, False), (b, 1, occ, False)]
        elif name == 'coincident':
            # the target at the ego's own place (a = 0: the a_safe branch), and two entities at one place
            state[b, ego, :2] = base
            state[b, tgt, :2] = base
            state[b, occ, :2] = base + np.array([20.0, 0.0])
            state[b, occ - 1, :2] = state[b, occ, :2]
            size[b, [occ, occ - 1], 1] = 2.0
            marks += [(b, ego, tgt, True)]          # a = 0, b = 0: the discriminant is 0 for ANY occluder, t = 0 / 2e-8 = 0: hidden
        elif name == 'tangent':
            # ego (0,0), target (10,0), occluder (5,1), width 2: the sight line touches the disc, discriminant 0 exactly; scaled by 2^b
            s = 2.0 ** b
            state[b, ego, :2], state[b, tgt, :2], state[b, occ, :2] = base, base + s * np.array([10.0, 0.0]), base + s * np.array([5.0, 1.0])
            size[b, occ, 1] = 2.0 * s
            # and just clear of it (width 2 - 1/8)
            state[b, tgt - 1, :2], state[b, occ - 1, :2] = base + s * np.array([0.0, 10.0]), base + s * np.array([1.0, 5.0])
            size[b, occ - 1, 1] = (2.0 - 0.125) * s
            marks += [(b, ego, tgt, True), (b, ego, tgt - 1, False)]
        elif name == 'zero_width':
            # a zero-width occluder hides only what is exactly behind its centre
            state[b, ego, :2], state[b, occ, :2], state[b, tgt, :2] = base, base + np.array([4.0, 0.0]), base + np.array([8.0, 0.0])
            state[b, occ - 1, :2], state[b, tgt - 1, :2] = base + np.array([0.25, 4.0]), base + np.array([0.0, 8.0])
            size[b, [occ, occ - 1], 1] = 0.0
            size[b, gen.uniform(size=E) < 0.3, 1] = 0.0
            marks += [(b, ego, tgt, True), (b, ego, tgt - 1, False)]
        elif name == 'absent_occluder':
            # an absent entity still hides what is behind it, as in the reference (observation_noise.py:89-132 masks targets only)
            state[b, ego, :2], state[b, occ, :2], state[b, tgt, :2] = base, base + np.array([6.0, 2.0]), base + np.array([12.0, 4.0])
            present[b, occ] = False
            present[b, tgt] = True
            marks += [(b, ego, tgt, True)]
        elif name == 'nan_row':
            # a NaN occluder hides nothing and a NaN target is never hidden; in the last scene the ego itself is NaN
            state[b, ego, :2], state[b, occ, :2], state[b, tgt, :2] = base, base + np.array([6.0, 2.0]), base + np.array([12.0, 4.0])
            state[b, occ] = np.nan
            state[b, tgt - 1] = np.nan
            marks += [(b, ego, tgt, False), (b, ego, tgt - 1, False)]
            if b == B - 1:
                state[b, A - 1] = np.nan
        present[b, [ego, tgt, tgt - 1]] = True
    return state.astype(np.float32), size.astype(np.float32), present, marks


def check_conditions(B, A, E, name, state, size, present, marks, mask):
    """judged on the inputs and on the oracle's mask alone"""
    assert mask.shape == (B, A, E)
    assert not (mask & ~present[:, None, :]).any()
    if name == 'random' and E > 1:
        visible = mask[np.broadcast_to(present[:, None, :], mask.shape)].mean()
        assert 0.1 <= visible <= 0.9, visible
    if E == 1:
        assert np.array_equal(mask, present[:, None, :])
    for b, a, e, hidden in marks:
        assert present[b, e] and bool(mask[b, a, e]) != hidden, (name, b, a, e, hidden)
    if name != 'random' and E >= MIN_E:
        assert len(marks) >= B
    if name == 'coincident' and E >= MIN_E:
        assert (state[:, 0, :2] == state[:, E - 1, :2]).all() and (state[:, E // 2, :2] == state[:, E // 2 - 1, :2]).all()
    if name == 'nan_row' and E >= MIN_E:
        assert np.isnan(state[:, :A]).any() and np.isnan(state[:, E // 2]).all()
