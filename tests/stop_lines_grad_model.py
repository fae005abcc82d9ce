"""Float64 autograd model of the differentiable stop-line observations (include/tdship.h "K7b").

`features` writes the eight features of K7 in torch, slot by slot, in float64 or float32; the gradients come from torch autograd
(`scene_gradients`).  The model takes `index` as given -- which line is in a slot is a constant of differentiation -- and shares no code with the
kernel's header csrc/tds_stop_lines_grad.h: the formulas of the backward are nowhere in this file.  The one thing it states beyond K7 is the
definition's own convention for an observer exactly on a line's centre: the distance contributes no gradient there."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64


def filled_slots(index, N):
    """the slots that hold a line: 0 <= n < N -> (filled (B,A,K) bool, b, a, k, n)"""
    index = np.asarray(index).astype(np.int64)
    filled = (index >= 0) & (index < N)
    b, a, k = np.nonzero(filled)
    return filled, b, a, k, index[b, a, k]


def features(P, L, b, a, n):
    """P (B,A,4) [x, y, sin, cos] of the observers, L (B,N,7) [x, y, length, width, sin, cos, time to change] of the lines, torch; b, a, n index
    tensors of m slots -> (m, 8), the features of K7"""
    xa, ya, s, c = P[b, a].unbind(-1)
    xn, yn, ln, wn, sl, cl, tn = L[b, n].unbind(-1)
    dx, dy = xn - xa, yn - ya
    d2 = dx * dx + dy * dy
    on = d2 > 0
    dist = torch.where(on, torch.sqrt(torch.where(on, d2, torch.ones_like(d2))), torch.zeros_like(d2))     # no gradient from a distance of 0
    return torch.stack([dx * c + dy * s, dy * c - dx * s, sl * c - cl * s, cl * c + sl * s, ln, wn, tn, dist], -1)


def scene_gradients(agent_xy, agent_sc, lines, line_sc, index, g, dtype=torch.float64, time_to_change=None):
    """the backward of a whole call by autograd: agent_xy, agent_sc (B,A,2), lines (B,N,5), line_sc (B,N,2) float32 as the kernel read them, index
    (B,A,K) as the forward wrote it, g (B,A,K,8) the incoming gradient -> g_xy (B,A,2), g_sc (B,A,2) float64 numpy, filled (B,A,K) bool.  The
    formula runs in `dtype` on the inputs widened (float64) or as they are (float32).  What comes in at a slot that is not filled is never read;
    the lines are leaves without grad: they are constants."""
    agent_xy, agent_sc, lines, line_sc = (np.asarray(v, F32) for v in (agent_xy, agent_sc, lines, line_sc))
    B, A = agent_xy.shape[:2]
    N = lines.shape[1]
    ttc = np.zeros((B, N), F32) if time_to_change is None else np.asarray(time_to_change, F32)
    filled, b, a, k, n = filled_slots(index, N)
    grad = np.zeros((B, A, 4))
    if len(b):
        P = torch.tensor(np.concatenate([agent_xy, agent_sc], -1).astype(F64)).to(dtype).requires_grad_(True)
        L = torch.tensor(np.concatenate([lines[..., :4], line_sc, ttc[..., None]], -1).astype(F64)).to(dtype)
        tb, ta, tn = (torch.as_tensor(v) for v in (b, a, n))
        gin = torch.as_tensor(np.asarray(g, F32)[b, a, k]).to(dtype)
        # a NaN that comes in at g4 .. g6 of a filled slot meets a constant: it must not reach the sum
        f = features(P, L, tb, ta, tn)
        live = [0, 1, 2, 3, 7]
        (f[:, live] * gin[:, live]).sum().backward()
        grad = P.grad.double().numpy()
    return grad[..., :2].copy(), grad[..., 2:].copy(), filled


def chain_state(g_xy, g_sc, sc, dtype=F64):
    """the gradient of the state [x, y, psi, v]: psi through [sin, cos] = the values `sc` the kernel read -> (B,A,4)"""
    s, c = np.asarray(sc)[..., 0].astype(dtype), np.asarray(sc)[..., 1].astype(dtype)
    gs, gc = g_sc[..., 0].astype(dtype), g_sc[..., 1].astype(dtype)
    return np.stack([g_xy[..., 0], g_xy[..., 1], (gs * c - gc * s).astype(F64), np.zeros_like(g_xy[..., 0])], -1)


def observers(filled):
    """(B,A) bool: the observers with a filled slot; every other row of both gradients is exactly zero"""
    return filled.any(-1)
