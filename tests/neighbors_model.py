"""Brute-force numpy model of the neighbour observations (include/tdship.h "K6"): binary32 throughout, the operations of the
definition in its order, each rounded once -- numpy float32 arithmetic does not contract -- so the kernel (csrc/neighbors.hip) must equal it
bit for bit.  `neighbors64` restates the definition in float64 for tests/test_neighbors_model.py."""
import numpy as np

MAX_K, MAX_ENTITIES = 32, 1024
F32 = np.float32


def neighbors(boxes, sc, speed, present, n_exposed, k, max_distance, visible=None):
    """boxes (B,E,5), sc (B,E,2), speed (B,E), present (B,E), visible None or (B,A,E) -> features (B,A,k,8) float32, index (B,A,k) int32"""
    boxes, sc, speed = np.asarray(boxes, F32), np.asarray(sc, F32), np.asarray(speed, F32)
    present = np.asarray(present).astype(bool)
    B, E = boxes.shape[:2]
    A, K = int(n_exposed), int(k)
    assert 1 <= K <= MAX_K and A <= E <= MAX_ENTITIES and not (F32(max_distance) < 0) and not np.isnan(max_distance)
    with np.errstate(over='ignore', invalid='ignore'):
        r2 = F32(max_distance) * F32(max_distance)
        features = np.zeros((B, A, K, 8), F32)
        index = np.full((B, A, K), -1, np.int32)
        ents = np.arange(E)
        for b in range(B):
            x, y = boxes[b, :, 0], boxes[b, :, 1]
            for a in range(A):
                if not present[b, a]:
                    continue
                dx, dy = x - x[a], y - y[a]
                d2 = dx * dx + dy * dy
                cand = present[b] & (ents != a) & (d2 <= r2)                 # (a NaN d2 fails the comparison)
                if visible is not None:
                    cand &= np.asarray(visible[b, a]) != 0
                who = ents[cand]
                who = who[np.lexsort((who, d2[cand]))][:K]                   # by d2, equal d2 by the lower entity index
                n = len(who)
                s, c = sc[b, a, 0], sc[b, a, 1]
                se, ce = sc[b, who, 0], sc[b, who, 1]
                ddx, ddy = dx[who], dy[who]
                sin_rel, cos_rel = se * c - ce * s, ce * c + se * s
                f = features[b, a, :n]
                f[:, 0], f[:, 1] = ddx * c + ddy * s, ddy * c - ddx * s
                f[:, 2], f[:, 3] = sin_rel, cos_rel
                f[:, 4], f[:, 5] = speed[b, who] * cos_rel - speed[b, a], speed[b, who] * sin_rel
                f[:, 6], f[:, 7] = boxes[b, who, 2], boxes[b, who, 3]
                index[b, a, :n] = who
    return features, index


def features64(boxes, sc, speed, b, a, who, dtype=np.float64):
    """the eight features of the entities `who` seen from observer a of scene b, in float64 on the float32 inputs -> (len(who), 8); a restatement
    of the formulas that shares no code with `neighbors` (dtype=np.float32: the float32 yardstick of tests/test_neighbors_model.py)"""
    boxes, sc, speed = np.asarray(boxes, dtype), np.asarray(sc, dtype), np.asarray(speed, dtype)
    dx, dy = boxes[b, who, 0] - boxes[b, a, 0], boxes[b, who, 1] - boxes[b, a, 1]
    s, c = sc[b, a]
    se, ce = sc[b, who, 0], sc[b, who, 1]
    sin_rel, cos_rel = se * c - ce * s, ce * c + se * s
    return np.stack([dx * c + dy * s, dy * c - dx * s, sin_rel, cos_rel, speed[b, who] * cos_rel - speed[b, a], speed[b, who] * sin_rel,
                     boxes[b, who, 2], boxes[b, who, 3]], -1)


def heading_sc(psi):
    """[sin, cos] as float32 (the kernel takes them as an input: any values will do for a comparison)"""
    return np.stack([np.sin(psi.astype(np.float64)), np.cos(psi.astype(np.float64))], -1).astype(F32)


def definition_cases():
    """B = 2, A = 3, E = 5, to be asked for K = 4 within DEFINITION_MAX_DISTANCE -> dict(boxes, sc, speed, present).
    scene 0: observer 0 at the origin; entities 1 and 2 mirrored across its x axis (bit-equal d2 = 25: 1 comes first); entity 3 at d2 = 100 = r2
             exactly (in); entity 4 at d2 = the next float32 after 100 (out): observer 0 has 3 candidates for 4 slots.
    scene 1: observer 0 is absent (an empty row, and nobody's neighbour); observer 2 stands on observer 1 (d2 = 0); entity 3 has a NaN pose
             (never a candidate); entity 4 is an absent NPC next to them."""
    boxes = np.zeros((2, 5, 5), F32)
    boxes[..., 2], boxes[..., 3] = [4.5, 4.0, 5.0, 12.0, 0.9], [1.9, 1.8, 2.0, 2.5, 1.7]
    boxes[0, :, :2] = [[0, 0], [3, 4], [3, -4], [6, 8], [np.nextafter(F32(6), F32(7)), 8]]
    boxes[0, :, 4] = [0.3, -2.0, 1.0, 3.0, 0.0]
    boxes[1, :, :2] = [[1.5, 0.5], [1, 1], [1, 1], [np.nan, 2], [2, 1]]
    boxes[1, :, 4] = [0.0, 0.7, -0.7, 0.1, 2.0]
    present = np.ones((2, 5), bool)
    present[1, 0] = present[1, 4] = False
    speed = np.array([[5.0, 3.0, 0.0, 7.5, 1.0], [2.0, 4.0, 6.0, 1.0, 3.0]], F32)
    d2 = boxes[0, 4, 0] * boxes[0, 4, 0] + boxes[0, 4, 1] * boxes[0, 4, 1]
    assert d2 == np.nextafter(F32(100), F32(200)) and F32(DEFINITION_MAX_DISTANCE) * F32(DEFINITION_MAX_DISTANCE) == F32(100)
    return dict(boxes=boxes, sc=heading_sc(boxes[..., 4]), speed=speed, present=present)


DEFINITION_MAX_DISTANCE = 10.0
#: the index tensor of definition_cases() at K = 4, by hand from the definition
DEFINITION_INDEX = [[[1, 2, 3, -1], [0, 3, 4, 2], [0, 1, -1, -1]], [[-1, -1, -1, -1], [2, -1, -1, -1], [1, -1, -1, -1]]]


def random_scenes(seed, B, A, E, side=120.0, duplicates=0.1, absent=0.1):
    """float32 poses in a square of `side` metres; a share of the entities stands exactly on another one (d2 = 0 for that pair, bit-equal d2 for
    everybody else) and a share is absent -> dict(boxes, sc, speed, present)"""
    g = np.random.default_rng(seed)
    boxes = np.concatenate([g.uniform(0, side, (B, E, 2)), g.uniform(3.5, 6.0, (B, E, 1)), g.uniform(1.6, 2.4, (B, E, 1)), g.uniform(-np.pi, np.pi, (B, E, 1))],
                           -1).astype(F32)
    for b in range(B):
        for e in np.nonzero(g.random(E) < duplicates)[0]:
            boxes[b, e, :2] = boxes[b, g.integers(E), :2]
    return dict(boxes=boxes, sc=heading_sc(boxes[..., 4]), speed=g.uniform(0, 15, (B, E)).astype(F32), present=g.random((B, E)) >= absent)


def d2_64(boxes, b, a):
    """float64 squared distances of every entity of scene b from observer a, on the float32 inputs"""
    boxes = np.asarray(boxes, np.float64)
    return (boxes[b, :, 0] - boxes[b, a, 0]) ** 2 + (boxes[b, :, 1] - boxes[b, a, 1]) ** 2
