"""
Torch-autograd model of the differentiable route step (csrc/route_bwd.hip, csrc/tds_route_grad.h; DESIGN.md 5.5f, include/tdship.h), one row at a
time.  The DISCRETE choices of the forward -- the piece, the segment, which clamp is active, the lookahead's pieces and segments -- are taken
from route_model.progress and are constants; the CONTINUOUS arithmetic is restated here on torch scalars in the definition's order, and autograd
differentiates it.  In float64 the forward equals route_model.progress(exact=True) bit for bit (tests/test_route_grad_model.py).  `dtype` =
torch.float32 gives the float32 yardstick of the GPU tests: the same choices (made in float64), every constant and every operation in float32.
"""
import copy
import math

import numpy as np
import torch

import route_model as rm

FLOATS = ('progress', 'advance', 'lateral', 'heading', 'remaining', 'lookahead')


def choices(lanes, route, x, y, sn, cs, K=16, spacing=4.0, present=True):
    """The forward of one row on a COPY of the route (the route itself is not moved): None for a row without a foot, else a dict of
    route_model.progress's float64 outputs (`out`), the foot's `piece` and `segment`, its `clamp` (-1: at ulo, 0: interior, 1: at uhi) and per
    lookahead point `look` = (piece, segment, q moves with progress)."""
    moved = copy.copy(route)
    out = rm.progress(lanes, moved, x, y, sn, cs, K=K, spacing=spacing, present=present, exact=True)
    if not out['found']:
        return None
    x, y = float(x), float(y)
    j, i = out['piece'], out['segment']
    c, cum = lanes.cl[route.lanes[j]], lanes.cum[route.lanes[j]]
    a, b = route.interval(lanes, j)
    px, py = float(c[i][0]), float(c[i][1])
    dx, dy = float(c[i + 1][0]) - px, float(c[i + 1][1]) - py
    w = cum[i + 1] - cum[i]
    ulo = (a - cum[i]) / w if a > cum[i] else 0.0
    uhi = (b - cum[i]) / w if b < cum[i + 1] else 1.0
    u_raw = ((x - px) * dx + (y - py) * dy) / (dx * dx + dy * dy)
    clamp = -1 if u_raw < ulo else 1 if u_raw > uhi else 0
    if not rm.weigh_segment(c, cum, i, a, b, x, y)[1] < math.inf:            # a pose no segment can be weighed against (NaN): the kernels find no foot
        return None
    look = []
    for m in range(K):
        q = out['progress'] + float(m + 1) * float(rm.F32(spacing))
        moves = q > 0.0 and q <= route.length
        q = min(max(q, 0.0), route.length) if q > 0.0 else 0.0
        pj = 0
        for k in range(1, route.n):
            if route.offsets[k] <= q:
                pj = k
        arc = (route.start_arc if pj == 0 else 0.0) + (q - route.offsets[pj])
        look.append((pj, lanes.segment_of(route.lanes[pj], arc), moves))
    return dict(out=out, piece=j, segment=i, clamp=clamp, ulo=ulo, uhi=uhi, look=look, stored=route.stored)


def forward(lanes, route, xy, sc, K=16, spacing=4.0, present=True, dtype=torch.float64):
    """-> (pose, [sin, cos], outputs): two leaf tensors of `dtype` that require grad and the dict of the six float outputs computed from them; the
    outputs are None for a row without a foot (every gradient is zero there).  xy, sc: two float32 values each."""
    ch = choices(lanes, route, xy[0], xy[1], sc[0], sc[1], K, spacing, present)
    pose = torch.tensor([float(xy[0]), float(xy[1])], dtype=dtype, requires_grad=True)
    heading = torch.tensor([float(sc[0]), float(sc[1])], dtype=dtype, requires_grad=True)
    if ch is None:
        return pose, heading, None
    k = lambda v: torch.tensor(float(v), dtype=dtype)                        # a constant of the row
    x, y, sn, cs = pose[0], pose[1], heading[0], heading[1]
    j, i = ch['piece'], ch['segment']
    c, cum = lanes.cl[route.lanes[j]], lanes.cum[route.lanes[j]]
    a, _ = route.interval(lanes, j)
    p0, p1 = k(c[i][0]), k(c[i][1])
    dx, dy = k(c[i + 1][0]) - p0, k(c[i + 1][1]) - p1
    l2 = dx * dx + dy * dy
    w = k(cum[i + 1]) - k(cum[i])
    u = ((x - p0) * dx + (y - p1) * dy) / l2
    if dtype == torch.float64:
        u = torch.clamp(u, k(ch['ulo']), k(ch['uhi']))                       # min(max(u, ulo), uhi); passes the gradient iff ulo <= u <= uhi
    elif ch['clamp']:                                                        # the float64 choice of the active clamp, kept in float32
        u = k(ch['ulo'] if ch['clamp'] < 0 else ch['uhi'])
    arc = k(cum[i]) + u * w
    progress = k(route.offsets[j]) + (arc - k(a))
    length = k(route.length)
    l = torch.sqrt(l2)
    tx, ty = dx / l, dy / l
    out = dict(progress=progress, advance=progress - k(ch['stored']), remaining=length - progress, lateral=tx * (y - p1) - ty * (x - p0),
               heading=torch.stack([sn * tx - cs * ty, cs * tx + sn * ty]))
    look = []
    for m, (pj, pk, moves) in enumerate(ch['look']):
        q = progress + k(m + 1) * k(rm.F32(spacing))
        q64 = ch['out']['progress'] + float(m + 1) * float(rm.F32(spacing))
        q = torch.where(torch.tensor(q64 > 0.0), q, k(0.0))                  # route_point's two clamps, as `where`s on the float64 decisions
        q = torch.where(torch.tensor(max(q64, 0.0) > route.length), length, q)
        pc, pcum = lanes.cl[route.lanes[pj]], lanes.cum[route.lanes[pj]]
        parc = k(route.start_arc if pj == 0 else 0.0) + (q - k(route.offsets[pj]))
        pw = k(pcum[pk + 1]) - k(pcum[pk])
        pu = (parc - k(pcum[pk])) / pw if pcum[pk + 1] - pcum[pk] > 0.0 else k(0.0)
        q0, q1 = k(pc[pk][0]), k(pc[pk][1])
        px, py = q0 + pu * (k(pc[pk + 1][0]) - q0), q1 + pu * (k(pc[pk + 1][1]) - q1)
        ex, ey = px - x, py - y
        look.append(torch.stack([ex * cs + ey * sn, ey * cs - ex * sn]))
    out['lookahead'] = torch.stack(look) if look else torch.zeros((0, 2), dtype=dtype)
    return pose, heading, out


def gradients(lanes, route, xy, sc, grads, K=16, spacing=4.0, present=True, dtype=torch.float64):
    """The gradient of sum over the outputs of <output, grads[name]> (a missing name or None: zero) -> (g_xy, g_sc), two float64 arrays of two."""
    pose, heading, out = forward(lanes, route, xy, sc, K, spacing, present, dtype)
    loss = None
    if out is not None:
        for name in FLOATS:
            g = grads.get(name)
            if g is not None and out[name].numel() > 0:
                term = (out[name] * torch.as_tensor(np.asarray(g, np.float64)).to(dtype)).sum()
                loss = term if loss is None else loss + term
    if loss is None or loss.grad_fn is None:
        return np.zeros(2), np.zeros(2)
    g_xy, g_sc = torch.autograd.grad(loss, (pose, heading), allow_unused=True)
    return tuple(np.zeros(2) if g is None else g.to(torch.float64).numpy() for g in (g_xy, g_sc))
