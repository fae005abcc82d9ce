"""Float64 autograd model of the differentiable neighbour observations (include/tdship.h "K6b").

`features` writes the eight features of K6 in torch, slot by slot, in float64 or float32; the gradients come from torch autograd
(`scene_gradients`).  The model takes `index` as given -- which entity is in a slot is a constant of differentiation -- and shares no code with
the kernel's header csrc/tds_neighbors_grad.h: the formulas of the backward are nowhere in this file."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
NAMES = ('x', 'y', 'length', 'width', 'sin', 'cos', 'speed')


def filled_slots(index, E):
    """the slots that hold an entity: 0 <= e < E and e is not the observer itself -> (filled (B,A,K) bool, b, a, k, e)"""
    index = np.asarray(index).astype(np.int64)
    a_of = np.arange(index.shape[1])[None, :, None]
    filled = (index >= 0) & (index < E) & (index != a_of)
    b, a, k = np.nonzero(filled)
    return filled, b, a, k, index[b, a, k]


def features(V, b, a, e):
    """V (B,E,7) [x, y, length, width, sin, cos, speed] torch; b, a, e index tensors of n slots -> (n, 8), the features of K6"""
    xa, ya, _, _, s, c, va = V[b, a].unbind(-1)
    xe, ye, le, we, se, ce, ve = V[b, e].unbind(-1)
    dx, dy = xe - xa, ye - ya
    sin_rel, cos_rel = se * c - ce * s, ce * c + se * s
    return torch.stack([dx * c + dy * s, dy * c - dx * s, sin_rel, cos_rel, ve * cos_rel - va, ve * sin_rel, le, we], -1)


def scene_gradients(boxes, sc, speed, index, g, dtype=torch.float64):
    """the backward of a whole call by autograd: boxes (B,E,5), sc (B,E,2), speed (B,E) float32 as the kernel read them, index (B,A,K) as it wrote
    it, g (B,A,K,8) the incoming gradient -> g_boxes (B,E,5), g_sc (B,E,2), g_speed (B,E) float64 numpy, filled (B,A,K) bool.  The formula runs
    in `dtype` on the inputs widened (float64) or as they are (float32).  What comes in at a slot that is not filled is never read."""
    boxes, sc, speed = np.asarray(boxes, F32), np.asarray(sc, F32), np.asarray(speed, F32)
    B, E = boxes.shape[:2]
    V = np.concatenate([boxes[..., :4], sc, speed[..., None]], -1).astype(F64)
    filled, b, a, k, e = filled_slots(index, E)
    grad = np.zeros((B, E, 7))
    if len(b):
        X = torch.tensor(V).to(dtype).requires_grad_(True)
        tb, ta, te = (torch.as_tensor(v) for v in (b, a, e))
        gin = torch.as_tensor(np.asarray(g, F32)[b, a, k]).to(dtype)
        (features(X, tb, ta, te) * gin).sum().backward()
        grad = X.grad.double().numpy()
    g_boxes = np.concatenate([grad[..., :4], np.zeros((B, E, 1))], -1)
    return g_boxes, grad[..., 4:6].copy(), grad[..., 6].copy(), filled


def chain_state(g_boxes, g_sc, g_speed, sc, dtype=F64):
    """the gradient of the state [x, y, psi, v]: psi through [sin, cos] = the values `sc` the kernel read -> (B,E,4)"""
    s, c = np.asarray(sc)[..., 0].astype(dtype), np.asarray(sc)[..., 1].astype(dtype)
    gs, gc = g_sc[..., 0].astype(dtype), g_sc[..., 1].astype(dtype)
    return np.stack([g_boxes[..., 0], g_boxes[..., 1], (gs * c - gc * s).astype(F64), g_speed], -1)


def touched(filled, index, E):
    """(B,E) bool: the entities that a filled slot touches, as its observer or as its entity"""
    out = np.zeros((filled.shape[0], E), bool)
    b, a, k = np.nonzero(filled)
    out[b, a] = True
    out[b, np.asarray(index)[b, a, k]] = True
    return out


#: the device tests' scenes: name -> (seed, B, A, E, K, max_distance), and the filled slots each must have at least
CASES = {'E6': (6, 3, 3, 6, 4, 50.0), 'E64': (64, 2, 64, 64, 4, 50.0), 'E65': (65, 2, 40, 65, 4, 50.0), 'E33': (33, 2, 17, 33, 4, 50.0),
         'E130': (130, 2, 70, 130, 8, 30.0), 'E1024': (1024, 1, 2, 1024, 32, float('inf'))}
FILLED = {'E6': 8, 'E64': 456, 'E65': 288, 'E33': 132, 'E130': 1008, 'E1024': 64}
