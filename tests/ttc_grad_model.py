"""Float64 autograd model of differentiable time to collision (include/tdship.h "K9b").

Three parts.  `pair_choices` takes the forward's discrete choices -- whether the pair contributes, the binding axis, the sign of w on it, the signs of
the four fabs arguments of R -- from numpy float64 in the arithmetic of tests/ttc_model.py.  `times` writes the chosen branch t = (-sigma R - p) / w
in torch, with those choices as constants, in float64 or float32; the gradients come from torch autograd (`pair_gradients`, `scene_gradients`).
`pair_partials` is the numpy restatement of csrc/tds_ttc_grad.h, operation for operation in the header's order: the host build of the header must
equal it bit for bit (tests/test_ttc_grad_host.py), and it is itself held to the autograd model (tests/test_ttc_grad_model.py)."""
import numpy as np
import torch

import ttc_model as tm

F32, F64 = np.float32, np.float64
NAMES = ('x', 'y', 'length', 'width', 'sin', 'cos', 'speed')


def sign(v):
    """-1, 0 or 1 as float64; sign(0) = +0.0"""
    return (v > 0).astype(F64) - (v < 0).astype(F64)


def axes_of(a, e):
    (xa, ya, la, wa, sa, ca, va), (xe, ye, le, we, se, ce, ve) = a, e
    return ((ca, sa), (-sa, ca), (ce, se), (-se, ce))


def pair_choices(a, e, margin=0.0):
    """a, e: the seven values (x, y, l, w, s, c, v) of the observers and of the others, arrays of n, float64 and finite -> dict: contributes (n,)
    bool (lo > 0), lo, axis (the first axis whose t0 equals lo), w on it, and its (nx, ny)"""
    a = [np.asarray(v, F64) for v in a]
    e = [np.asarray(v, F64) for v in e]
    a = [np.broadcast_to(v, np.broadcast(*a, *e).shape) for v in a]
    e = [np.broadcast_to(v, a[0].shape) for v in e]
    (xa, ya, la, wa, sa, ca, va), (xe, ye, le, we, se, ce, ve) = a, e
    margin = F64(margin)
    hla, hwa = F64(0.5) * la + margin, F64(0.5) * wa + margin
    hle, hwe = F64(0.5) * le, F64(0.5) * we
    dx, dy = xe - xa, ye - ya
    rvx, rvy = ve * ce - va * ca, ve * se - va * sa
    n = dx.shape
    lo, wb, axis = np.full(n, -np.inf), np.zeros(n), np.zeros(n, int)
    with np.errstate(all='ignore'):
        for i, (nx, ny) in enumerate(axes_of(a, e)):
            p = dx * nx + dy * ny
            w = rvx * nx + rvy * ny
            R = hla * np.abs(ca * nx + sa * ny) + hwa * np.abs(ca * ny - sa * nx) + hle * np.abs(ce * nx + se * ny) + hwe * np.abs(ce * ny - se * nx)
            still = w == 0
            ws = np.where(still, 1.0, w)
            t0, t1 = (-R - p) / ws, (R - p) / ws
            t0 = np.where(t0 > t1, t1, t0)
            better = ~still & (t0 > lo)
            lo, wb, axis = np.where(better, t0, lo), np.where(better, w, wb), np.where(better, i, axis)
    ax = axes_of(a, e)
    nx = np.choose(axis, [np.broadcast_to(q[0], n) for q in ax])
    ny = np.choose(axis, [np.broadcast_to(q[1], n) for q in ax])
    return dict(contributes=lo > 0, lo=lo, axis=axis, w=wb, nx=nx, ny=ny, a=a, e=e, hl=(hla, hwa, hle, hwe), d=(dx, dy), rv=(rvx, rvy))


def pair_partials(a, e, margin=0.0):
    """csrc/tds_ttc_grad.h restated: -> (contributes (n,) bool, ga (n, 7), ge (n, 7)); the rows of pairs that do not contribute are 0"""
    ch = pair_choices(a, e, margin)
    (xa, ya, la, wa, sa, ca, va), (xe, ye, le, we, se, ce, ve) = ch['a'], ch['e']
    (hla, hwa, hle, hwe), (dx, dy), (rvx, rvy) = ch['hl'], ch['d'], ch['rv']
    ok, axis, nx, ny = ch['contributes'], ch['axis'], ch['nx'], ch['ny']
    half = F64(0.5)
    with np.errstate(all='ignore'):
        wb = np.where(ok, ch['w'], 1.0)
        t = np.where(ok, ch['lo'], 0.0)
        sigma, inv = sign(wb), F64(-1.0) / wb
        a1, a2 = ca * nx + sa * ny, ca * ny - sa * nx
        e1, e2 = ce * nx + se * ny, ce * ny - se * nx
        ka1, ka2 = sigma * (hla * sign(a1)), sigma * (hwa * sign(a2))
        ke1, ke2 = sigma * (hle * sign(e1)), sigma * (hwe * sign(e2))
        qx, qy = dx + t * rvx, dy + t * rvy
        gnx = ((ka1 * ca - ka2 * sa) + (ke1 * ce - ke2 * se)) + qx
        gny = ((ka1 * sa + ka2 * ca) + (ke1 * se + ke2 * ce)) + qy
        nca = (ka1 * nx + ka2 * ny) - t * (va * nx)
        nsa = (ka1 * ny - ka2 * nx) - t * (va * ny)
        nce = (ke1 * nx + ke2 * ny) + t * (ve * nx)
        nse = (ke1 * ny - ke2 * nx) + t * (ve * ny)
        nca, nsa = np.where(axis == 0, nca + gnx, np.where(axis == 1, nca + gny, nca)), np.where(axis == 0, nsa + gny, np.where(axis == 1, nsa - gnx, nsa))
        nce, nse = np.where(axis == 2, nce + gnx, np.where(axis == 3, nce + gny, nce)), np.where(axis == 2, nse + gny, np.where(axis == 3, nse - gnx, nse))
        gxe, gye = nx * inv, ny * inv
        ga = [-gxe, -gye, (sigma * (half * np.abs(a1))) * inv, (sigma * (half * np.abs(a2))) * inv, nsa * inv, nca * inv, -((t * a1) * inv)]
        ge = [gxe, gye, (sigma * (half * np.abs(e1))) * inv, (sigma * (half * np.abs(e2))) * inv, nse * inv, nce * inv, (t * e1) * inv]
    zero = lambda cols: np.where(ok[..., None], np.stack(cols, -1), 0.0)
    return ok, zero(ga), zero(ge)


# ---- the chosen branch in torch ---------------------------------------------------------------------------------------------------------
def times(A, O, ch, margin, dtype):
    """A, O: (n, 7) torch tensors of `dtype`, the observers and the others; ch: pair_choices of the same pairs (all of them contributing) ->
    (n,) the time of the forward's branch, t = (-sigma R - p) / w on the binding axis, every discrete choice a constant"""
    xa, ya, la, wa, sa, ca, va = A.unbind(-1)
    xe, ye, le, we, se, ce, ve = O.unbind(-1)
    const = lambda v: torch.as_tensor(np.asarray(v, F64)).to(dtype)
    axis = torch.as_tensor(np.asarray(ch['axis']))
    pick = lambda q: torch.where(axis == 0, q[0], torch.where(axis == 1, q[1], torch.where(axis == 2, q[2], q[3])))
    nx, ny = pick((ca, -sa, ce, -se)), pick((sa, ca, se, ce))
    cnx, cny = ch['nx'], ch['ny']
    (_, _, _, _, nsa, nca, _), (_, _, _, _, nse, nce, _) = ch['a'], ch['e']
    s1, s2 = const(sign(nca * cnx + nsa * cny)), const(sign(nca * cny - nsa * cnx))
    s3, s4 = const(sign(nce * cnx + nse * cny)), const(sign(nce * cny - nse * cnx))
    sigma = const(sign(ch['w']))
    m = float(F32(margin))
    hla, hwa, hle, hwe = 0.5 * la + m, 0.5 * wa + m, 0.5 * le, 0.5 * we
    dx, dy = xe - xa, ye - ya
    rvx, rvy = ve * ce - va * ca, ve * se - va * sa
    p = dx * nx + dy * ny
    w = rvx * nx + rvy * ny
    R = hla * (s1 * (ca * nx + sa * ny)) + hwa * (s2 * (ca * ny - sa * nx)) + hle * (s3 * (ce * nx + se * ny)) + hwe * (s4 * (ce * ny - se * nx))
    return (-sigma * R - p) / w


def pair_gradients(a, e, margin=0.0, dtype=torch.float64):
    """autograd on `times`, pair by pair: -> (contributes (n,), t (n,), ga (n, 7), ge (n, 7)) as float64 numpy; zeros where the pair does not
    contribute"""
    ch = pair_choices(a, e, margin)
    ok = ch['contributes']
    n = len(ok)
    t, ga, ge = np.zeros(n), np.zeros((n, 7)), np.zeros((n, 7))
    if ok.any():
        sub = {k: (v[ok] if isinstance(v, np.ndarray) else [q[ok] for q in v]) for k, v in ch.items()}
        A = torch.tensor(np.stack(sub['a'], -1)).to(dtype).requires_grad_(True)
        O = torch.tensor(np.stack(sub['e'], -1)).to(dtype).requires_grad_(True)
        tt = times(A, O, sub, margin, dtype)
        tt.sum().backward()
        t[ok], ga[ok], ge[ok] = tt.detach().double().numpy(), A.grad.double().numpy(), O.grad.double().numpy()
    return ok, t, ga, ge


def slots_of(boxes, sc, speed, index):
    """the slots that may contribute by their index and their values alone -> (V (B,E,7) float64 with non-finite entities zeroed, b, a, k, e)"""
    boxes, sc, speed = np.asarray(boxes, F32), np.asarray(sc, F32), np.asarray(speed, F32)
    index = np.asarray(index)
    B, E = boxes.shape[:2]
    V = np.concatenate([boxes[..., :4], sc, speed[..., None]], -1).astype(F64)
    finite = np.isfinite(V).all(-1)
    V = np.where(finite[..., None], V, 0.0)
    b, a, k = np.nonzero((index >= 0) & (index < E))
    e = index[b, a, k].astype(int)
    keep = (e != a) & finite[b, a] & finite[b, e]
    return V, b[keep], a[keep], k[keep], e[keep]


def scene_gradients(boxes, sc, speed, index, g_ttc, margin=0.0, dtype=torch.float64):
    """the backward of a whole call by autograd: boxes (B,E,5), sc (B,E,2), speed (B,E) float32 as the kernel read them, index (B,A,K) as it wrote
    it, g_ttc (B,A,K) -> g_boxes (B,E,5), g_sc (B,E,2), g_speed (B,E) float64 numpy, contributes (B,A,K) bool.  The formula runs in `dtype` on
    the inputs widened (float64) or as they are (float32); the choices are always the float64 ones."""
    V, b, a, k, e = slots_of(boxes, sc, speed, index)
    B, E = V.shape[:2]
    contributes = np.zeros(np.asarray(index).shape, bool)
    g = np.zeros((B, E, 7))
    if len(b):
        ch = pair_choices(list(V[b, a].T), list(V[b, e].T), F32(margin))
        ok = ch['contributes']
        b, a, k, e = b[ok], a[ok], k[ok], e[ok]
        contributes[b, a, k] = True
        if len(b):
            sub = {key: (v[ok] if isinstance(v, np.ndarray) else [q[ok] for q in v]) for key, v in ch.items()}
            X = torch.tensor(V).to(dtype).requires_grad_(True)
            tb, ta, te = (torch.as_tensor(v) for v in (b, a, e))
            t = times(X[tb, ta], X[tb, te], sub, margin, dtype)
            gin = torch.as_tensor(np.asarray(g_ttc, F32)[b, a, k]).to(dtype)
            (t * gin).sum().backward()
            g = X.grad.double().numpy()
    g_boxes = np.concatenate([g[..., :4], np.zeros((B, E, 1))], -1)
    return g_boxes, g[..., 4:6].copy(), g[..., 6].copy(), contributes


def chain_state(g_boxes, g_sc, g_speed, sc, dtype=F64):
    """the gradient of the state [x, y, psi, v]: psi through [sin, cos] = the values `sc` the kernel read -> (B,E,4)"""
    s, c = np.asarray(sc)[..., 0].astype(dtype), np.asarray(sc)[..., 1].astype(dtype)
    gs, gc = g_sc[..., 0].astype(dtype), g_sc[..., 1].astype(dtype)
    return np.stack([g_boxes[..., 0], g_boxes[..., 1], (gs * c - gc * s).astype(F64), g_speed], -1)


def pairs_values(pairs):
    """ttc_model.random_pairs' (n, 2, 6) [x, y, l, w, psi, v] -> (a, e): the seven float32 values of each side, widened, [sin, cos] rounded to
    float32 as the kernels read them"""
    q = np.asarray(pairs, F32)
    sc = tm.nm.heading_sc(q[..., 4])
    return [[z.astype(F64) for z in (q[:, side, 0], q[:, side, 1], q[:, side, 2], q[:, side, 3], sc[:, side, 0], sc[:, side, 1], q[:, side, 5])] for side in (0, 1)]
