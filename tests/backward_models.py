"""
The yardsticks of the hand-derived backward kernels (csrc/backward.hip: offroad_bwd_kernel, discs_pair_bwd under both collision backward
kernels; csrc/kinematic.hip: bicycle_step_bwd_kernel, simple_step_bwd_kernel, unicycle_step_bwd_kernel): plain torch restatements of the DEFINITIONS (oracle/tds_oracle.c
R3d / R4, the kernels' comments), differentiated by torch autograd on the CPU.  Brute force over all faces and all pairs -- no grid, no lists,
no hierarchy, no hand-written derivative, so they cannot share a bug with the kernels'.  Every function takes a `dtype`: float64 is the
reference, float32 the yardstick (what ANY float32 evaluation of the same formulas may differ from float64 by; tests/test_backward_models.py
prints that table, tests/test_gpu_backward_float64.py holds the kernels to 4 x it).

Inputs are the float32 tensors the kernels get ([sin, cos] of the heading included, for the off-road loss), cast to `dtype` first.

Also here, because the CPU tests (caps, yardsticks) and the GPU tests must see the SAME inputs: the generators of the input sets, and the
borderline flags -- rows at which the loss is not differentiable within rounding (a nearest face about to change, a distance at the threshold,
two disc centres at the same distance), computed from the float64 model alone, never from a kernel.
"""
import math

import numpy as np
import torch

from conftest import load_golden

F64, F32 = torch.float64, torch.float32


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to('cpu').to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# off-road
# ---------------------------------------------------------------------------------------------------------------------------------------
def crop_mesh(verts, faces, x0, x1, y0, y1):
    """the faces whose three vertices lie in [x0, x1] x [y0, y1], vertices re-indexed: (verts (V, 2) float32, faces (F, 3) int64)"""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    ok = (verts[:, 0] >= x0) & (verts[:, 0] <= x1) & (verts[:, 1] >= y0) & (verts[:, 1] <= y1)
    faces = faces[ok[faces].all(1)]
    used = np.unique(faces)
    index = np.full(len(verts), -1, np.int64)
    index[used] = np.arange(len(used))
    return np.ascontiguousarray(verts[used]), np.ascontiguousarray(index[faces])


CROP_A, CROP_B = (0.0, 120.0, -10.0, 110.0), (80.0, 220.0, -10.0, 130.0)          # 4 456 and 8 115 faces of Town01


def town_crop(box=CROP_A):
    t = load_golden('town01_mesh.npz')
    return crop_mesh(t['verts'], t['faces'], *box)


def box_corners(state, lenwid, sc):
    """(..., 4, 2): (+-l/2, +-w/2) rotated by [sin, cos] plus (x, y)"""
    sx = torch.tensor([0.5, -0.5, -0.5, 0.5], dtype=state.dtype)
    sy = torch.tensor([0.5, 0.5, -0.5, -0.5], dtype=state.dtype)
    lx, ly = sx * lenwid[..., 0:1], sy * lenwid[..., 1:2]
    s, c = sc[..., 0:1], sc[..., 1:2]
    return torch.stack([lx * c - ly * s + state[..., 0:1], lx * s + ly * c + state[..., 1:2]], -1)


def _segment_d2(px, py, ax, ay, bx, by):
    """clamped point-segment squared distance; a degenerate edge (l2 <= 1e-8) gives the distance to b"""
    ex, ey = bx - ax, by - ay
    l2 = ex * ex + ey * ey
    t = (ex * (px - ax) + ey * (py - ay)) / (l2 + 1e-8)
    tc = t.clamp(0.0, 1.0)                                       # (passes the gradient on [0, 1], ends included: as the kernel)
    rx, ry = px - (ax + tc * ex), py - (ay + tc * ey)
    return torch.where(l2 <= 1e-8, (px - bx) ** 2 + (py - by) ** 2, rx * rx + ry * ry)


def triangle_d2(px, py, tri):
    """squared distance of points (px, py) to triangles tri (..., 3, 2), broadcast against each other: 0 inside (barycentric test with the
    +1e-8 denominator; faces of area < 5e-3 or |cross| <= 1e-8 are never "inside"), else the least of the three edge distances"""
    x0, y0, x1, y1, x2, y2 = tri[..., 0, 0], tri[..., 0, 1], tri[..., 1, 0], tri[..., 1, 1], tri[..., 2, 0], tri[..., 2, 1]
    p0x, p0y, p1x, p1y, p2x, p2y = x1 - x0, y1 - y0, x2 - x0, y2 - y0, px - x0, py - y0
    cross = p1x * p0y - p1y * p0x
    d00, d01, d11 = p0x * p0x + p0y * p0y, p0x * p1x + p0y * p1y, p1x * p1x + p1y * p1y
    d20, d21 = p2x * p0x + p2y * p0y, p2x * p1x + p2y * p1y
    denom = d00 * d11 - d01 * d01 + 1e-8
    w1, w2 = (d11 * d20 - d01 * d21) / denom, (d00 * d21 - d01 * d20) / denom
    w0 = 1.0 - w1 - w2
    inside = (w0 >= 0) & (w0 <= 1) & (w1 >= 0) & (w1 <= 1) & (w2 >= 0) & (w2 <= 1)
    inside = inside & ~(cross.abs() / 2.0 < 5e-3) & (cross.abs() > 1e-8)
    edges = torch.stack([_segment_d2(px, py, x0, y0, x1, y1), _segment_d2(px, py, x0, y0, x2, y2), _segment_d2(px, py, x1, y1, x2, y2)])
    dist = edges.min(0).values
    return torch.where(inside, torch.zeros_like(dist), dist)


def nearest_face(points, tri, chunk=512):
    """(P,) index of the face nearest to every point (P, 2), over ALL faces tri (F, 3, 2) -- the lowest index among equals"""
    out = torch.empty(points.shape[0], dtype=torch.int64)
    with torch.no_grad():
        for i in range(0, points.shape[0], chunk):
            p = points[i:i + chunk]
            out[i:i + chunk] = triangle_d2(p[:, 0:1], p[:, 1:2], tri[None]).min(1).indices
    return out


def offroad_model(state, lenwid, sc, verts, faces, threshold, present=None, dtype=F64, with_corners=False):
    """The off-road loss: per corner the least squared distance over all faces, zero where it is not > threshold, summed over the 4 corners,
    times present.  state (..., 4), lenwid (..., 2), sc (..., 2) [sin, cos] -- three inputs of their own, cast to `dtype` unless they have it
    already (pass leaves of `dtype` to differentiate).  The minimum over the faces passes its gradient to ONE face, so the search over all faces
    runs without a graph, in chunks of points (bounded memory), and only the winning face of every corner is evaluated again for autograd:
    exactly what differentiating min-over-faces gives.  with_corners: also the (..., 4) per-corner distances (before the threshold)."""
    state, lenwid, sc = (x if torch.is_tensor(x) and x.dtype == dtype else _t(x, dtype) for x in (state, lenwid, sc))
    tri = _t(verts, dtype)[torch.as_tensor(np.asarray(faces, np.int64))]                      # F x 3 x 2
    cor = box_corners(state, lenwid, sc)                                                       # ... x 4 x 2
    flat = cor.reshape(-1, 2)
    win = tri[nearest_face(flat.detach(), tri)]                                                # P x 3 x 2
    d = triangle_d2(flat[:, 0], flat[:, 1], win).reshape(cor.shape[:-1])
    loss = torch.where(d > threshold, d, torch.zeros_like(d)).sum(-1)
    if present is not None:
        loss = loss * _t(present, dtype)
    return (loss, d.detach()) if with_corners else loss


def offroad_grads(inp, sc, verts, faces, threshold, dtype=F64, shift=(0.0, 0.0), sc_inside=False):
    """-> dict(loss, gstate (..., 4), glenwid, gsc, corners) as float64 tensors: autograd of sum(offroad_model * grad_out) in `dtype`.
    shift: the agents moved by (dx, dy) first (the borderline probes).  sc_inside: [sin, cos] taken from psi inside the model (the
    gradient of psi is then in gstate[..., 2], and gsc is None)."""
    state = _t(inp['state'], dtype).clone()
    state[..., 0] += shift[0]
    state[..., 1] += shift[1]
    state.requires_grad_(True)
    lenwid = _t(inp['lenwid'], dtype).requires_grad_(True)
    scl = torch.stack([torch.sin(state[..., 2]), torch.cos(state[..., 2])], -1) if sc_inside else _t(sc, dtype).requires_grad_(True)
    loss, cor = offroad_model(state, lenwid, scl, verts, faces, threshold, inp['present'], dtype, with_corners=True)
    grads = torch.autograd.grad((loss * _t(inp['grad_out'], dtype)).sum(), [state, lenwid] + ([] if sc_inside else [scl]), allow_unused=True)
    z = lambda g, like: torch.zeros_like(like, dtype=F64) if g is None else g.to(F64)
    return dict(loss=loss.detach().to(F64), gstate=z(grads[0], state), glenwid=z(grads[1], lenwid), gsc=None if sc_inside else z(grads[2], scl),
                corners=cor.to(F64))


OFFROAD_DELTA = 2e-3        # metres: about 60 float32 ulps of a 400 m coordinate, far above the kernel's corner rounding


def offroad_borderline(inp, sc, verts, faces, threshold, base=None, sc_inside=False):
    """(...,) bool, from the float64 model alone: agents whose position gradient moves by more than 1.25 x 8 x delta x |grad_out| when they
    are moved by +-delta along x or y.  Where the distance field is smooth each corner's gradient 2 r moves by at most 2 delta (the Hessian of a
    squared distance to a segment is 2 n n^T or 2 I), the four corners' sum by 8 delta: more means a nearest face, a clamp or the threshold
    changes within delta of the agent."""
    base = offroad_grads(inp, sc, verts, faces, threshold, F64, sc_inside=sc_inside) if base is None else base
    bound = 1.25 * 8 * OFFROAD_DELTA * _t(inp['grad_out'], F64).abs()
    flag = torch.zeros(bound.shape, dtype=torch.bool)
    for shift in ((OFFROAD_DELTA, 0.0), (-OFFROAD_DELTA, 0.0), (0.0, OFFROAD_DELTA), (0.0, -OFFROAD_DELTA)):
        g = offroad_grads(inp, sc, verts, faces, threshold, F64, shift=shift, sc_inside=sc_inside)
        flag |= (g['gstate'][..., :2] - base['gstate'][..., :2]).norm(dim=-1) > bound
    return flag


OFFROAD_GRADS = ('gstate', 'glenwid', 'gsc')


def offroad_reference(inp, sc, verts, faces, threshold, sc_inside=False):
    """What a kernel's gradients of one input set are judged by: g64 (the float64 model), g32 (the same in float32), borderline (...,) and
    yard: per gradient tensor the largest |g32 - g64| over the non-borderline rows"""
    g64 = offroad_grads(inp, sc, verts, faces, threshold, F64, sc_inside=sc_inside)
    g32 = offroad_grads(inp, sc, verts, faces, threshold, F32, sc_inside=sc_inside)
    flag = offroad_borderline(inp, sc, verts, faces, threshold, g64, sc_inside=sc_inside)
    keys = [k for k in OFFROAD_GRADS if g64[k] is not None]
    return dict(g64=g64, g32=g32, borderline=flag, yard={k: float((g32[k] - g64[k])[~flag].abs().max()) for k in keys})


def discs_reference(inp):
    """the same for the discs collision: out64, g64, g32 (B, N, 5), borderline (B, N), yard (one figure: the gradient with respect to the boxes)"""
    out64, g64 = discs_grads(inp, F64)
    _, g32 = discs_grads(inp, F32)
    flag = discs_borderline(inp)
    return dict(out64=out64, g64=g64, g32=g32, borderline=flag, yard=float((g32 - g64)[~flag].abs().max()))


def cpu_heading_sc(state):
    s = torch.as_tensor(state, dtype=F32)
    return torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1)


def _agents(gen, xy, shape):
    """state / lenwid / present / grad_out of agents at xy: about 10 % of the rows absent, about 10 % without an incoming gradient"""
    n = shape + (1,)
    state = np.concatenate([xy.reshape(shape + (2,)), gen.uniform(-np.pi, np.pi, n), np.zeros(n)], -1).astype(np.float32)
    lenwid = np.concatenate([gen.uniform(4, 5, n), gen.uniform(1.8, 2.2, n)], -1).astype(np.float32)
    present = gen.random(shape) >= 0.1
    grad_out = gen.uniform(0.5, 1.5, shape).astype(np.float32)
    grad_out[gen.random(shape) < 0.1] = 0.0
    return dict(state=state, lenwid=lenwid, present=present, grad_out=grad_out)


OFFROAD_SETS = ('near', 'edge', 'beyond')
OFFROAD_SEEDS = dict(near=101, edge=102, beyond=103)


def offroad_inputs(name, verts):
    """The input sets of the off-road tests, (4, 64) agents each, on the crop `verts`:
        near    at crop vertices + N(0, 3 m): the lists path along a real road edge
        edge    uniform over the crop's bounding box +- 60 m: the lists' grid ends 48 m out, so wavefronts mix lists and hierarchy
        beyond  50 .. 300 m beyond the bounding box: hierarchy (or grid rings) only"""
    gen = np.random.default_rng(OFFROAD_SEEDS[name])
    shape = (4, 64)
    n = shape[0] * shape[1]
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    if name == 'near':
        xy = verts[gen.integers(0, len(verts), n)] + gen.normal(0, 3.0, (n, 2))
    elif name == 'edge':
        xy = gen.uniform(lo - 60.0, hi + 60.0, (n, 2))
    else:
        cand = gen.uniform(lo - 300.0, hi + 300.0, (16 * n, 2))
        out = np.maximum(np.maximum(lo - cand, cand - hi), 0.0).max(1)                       # Chebyshev distance beyond the box
        xy = cand[out >= 50.0][:n]
        assert len(xy) == n
    return _agents(gen, xy, shape)


# ---------------------------------------------------------------------------------------------------------------------------------------
# discs collision
# ---------------------------------------------------------------------------------------------------------------------------------------
def _discs_parts(boxes, dtype):
    x, y, l, w, psi = boxes.unbind(-1)
    head = psi + (math.pi / 2) * (w > l).to(dtype)
    r = torch.minimum(l, w) / 2
    h = torch.maximum(l, w) / 2 - r
    k = torch.arange(-2, 3, dtype=dtype)
    off = k * h[..., None] / 2                                                               # B x N x 5
    cen = torch.stack([x[..., None] + off * torch.cos(head)[..., None], y[..., None] + off * torch.sin(head)[..., None]], -1)
    return cen, r


def discs_pairs(boxes, n_exposed=None, dtype=F64):
    """-> (dist (B, A, N, 25): the centre distances of every pair, zero distances clamped so that they carry no gradient; arg (B, A, N) of the
    relu: 1 - min dist / (r_i + r_j))"""
    boxes = boxes if torch.is_tensor(boxes) and boxes.dtype == dtype else _t(boxes, dtype)
    A = boxes.shape[1] if n_exposed is None else int(n_exposed)
    cen, r = _discs_parts(boxes, dtype)
    e = cen[:, :A, None, :, None, :] - cen[:, None, :, None, :, :]                           # B x A x N x 5 x 5 x 2
    d2 = (e * e).sum(-1).flatten(-2)
    dist = d2.clamp_min(1e-30).sqrt()           # (the clamp passes no gradient below it: a zero distance has none, the kernel tests d > 0)
    arg = 1.0 - dist.min(-1).values / (r[:, :A, None] + r[:, None, :])
    return dist, arg


def discs_collision_model(boxes, present, n_exposed=None, dtype=F64):
    """Simulator.compute_collision with the discs metric: boxes (B, N, 5) [x, y, length, width, psi], present (B, N) -> (B, A).
    o_ij = relu(1 - d_ij / (r_i + r_j)) * present_j over ALL j, self included; out_i = sum_j o_ij - max_j o_ij (no present_i factor)."""
    _, arg = discs_pairs(boxes, n_exposed, dtype)
    o = torch.relu(arg) * _t(present, dtype)[:, None, :]
    return o.sum(-1) - o.max(-1).values


def discs_grads(inp, dtype=F64):
    """-> (out (B, A), grad wrt boxes (B, N, 5)) as float64 tensors: autograd of sum(model * grad_out) in `dtype`"""
    boxes = _t(inp['boxes'], dtype).requires_grad_(True)
    out = discs_collision_model(boxes, inp['present'], inp['n_exposed'], dtype)
    g, = torch.autograd.grad((out * _t(inp['grad_out'], dtype)).sum(), boxes)
    return out.detach().to(F64), g.to(F64)


def discs_borderline(inp):
    """(B, N) bool, from the float64 model alone.  A pair (i exposed, j != i) is borderline when the relu's argument is within 1e-4 of 0, when
    it overlaps and the two smallest of its 25 centre distances are within 1e-4 m, or when its row's two largest masked overlaps are both > 0
    and within 1e-5 of each other (then every overlapping pair of the row); a box is borderline if it is in a borderline pair."""
    with torch.no_grad():
        dist, arg = discs_pairs(inp['boxes'], inp['n_exposed'], F64)
        B, A, N = arg.shape
        two = dist.sort(-1).values[..., :2]
        over = arg > 0
        pair = (arg.abs() < 1e-4) | (over & ((two[..., 1] - two[..., 0]) < 1e-4))
        o = torch.relu(arg) * _t(inp['present'], F64)[:, None, :]
        top = o.sort(-1, descending=True).values[..., :2]
        tie = (top[..., 1] > 0) & ((top[..., 0] - top[..., 1]) < 1e-5)
        pair |= tie[..., None] & over
        pair &= ~torch.eye(A, N, dtype=torch.bool)[None]          # (a box and itself: distance 0, never a gradient)
        box = torch.zeros(B, N, dtype=torch.bool)
        box[:, :A] |= pair.any(2)
        box |= pair.any(1)
    return box


def overlapping_pairs(inp):
    """number of (i exposed, j != i, j present) pairs with a positive overlap, in the float64 model"""
    with torch.no_grad():
        _, arg = discs_pairs(inp['boxes'], inp['n_exposed'], F64)
        A, N = arg.shape[1:]
        return int(((arg > 0) & ~torch.eye(A, N, dtype=torch.bool)[None] & torch.as_tensor(inp['present'])[:, None, :]).sum())


#: name -> (B, N, n_exposed, spread in metres, seed)
DISCS_SETS = dict(sparse=(8, 64, None, 60.0, 201), dense=(4, 64, None, 6.0, 202), npc=(4, 100, 40, 12.0, 203), rows=(2, 132, None, 40.0, 204))


def discs_inputs(name):
    """The input sets of the discs tests: 30 % of the boxes wider than long (the heading + pi/2 branch), no length == width, about 90 %
    present, a random incoming gradient with every 7th row zero.
        sparse  8 x 64 over 60 m            dense  4 x 64 within 6 m: thousands of overlapping pairs, several chunks of the pair table
        npc     4 x 100, 40 exposed, 12 m   rows   2 x 132 over 40 m: more than 16 384 pairs, the one-wavefront-per-row kernel"""
    B, N, n_exposed, spread, seed = DISCS_SETS[name]
    gen = np.random.default_rng(seed)
    xy = (gen.random((B, N, 2)) - 0.5) * spread
    length, width = 4 + gen.random((B, N)), 1.8 + 0.4 * gen.random((B, N))
    wide = gen.random((B, N)) < 0.3
    length, width = np.where(wide, width, length), np.where(wide, length, width)
    boxes = np.concatenate([xy, length[..., None], width[..., None], (gen.random((B, N, 1)) - 0.5) * 6], -1).astype(np.float32)
    assert (boxes[..., 2] != boxes[..., 3]).all()
    A = N if n_exposed is None else n_exposed
    grad_out = gen.uniform(0.5, 1.5, (B, A)).astype(np.float32)
    grad_out[:, ::7] = 0.0
    return dict(boxes=boxes, present=gen.random((B, N)) >= 0.1, n_exposed=n_exposed, grad_out=grad_out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# K1: the closed forms of csrc/kinematic.hip's forward kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
def simple_step_model(state, action, dt=0.1, norm=(20.0, 20.0, 10 * np.pi, 5.0), oriented=False):
    """state (..., 4) [x, y, psi, v], action (..., 4): state + action * norm * dt; oriented: the xy action rotated by psi first"""
    ax, ay = action[..., 0], action[..., 1]
    if oriented:
        c, s = torch.cos(state[..., 2]), torch.sin(state[..., 2])
        ax, ay = c * ax - s * ay, s * ax + c * ay
    return state + torch.stack([ax * norm[0], ay * norm[1], action[..., 2] * norm[2], action[..., 3] * norm[3]], -1) * dt


def unicycle_step_model(state, action, dt=0.1, max_acc=5.0, max_yaw_rate=1.0):
    """state (..., 4) [x, y, psi, v], action (..., 2) [acceleration, yaw rate], both normalised; the position moves with the NEW speed along the
    OLD heading"""
    x, y, psi, v = state.unbind(-1)
    v = v + action[..., 0] * max_acc * dt
    return torch.stack([x + v * torch.cos(psi) * dt, y + v * torch.sin(psi) * dt, psi + action[..., 1] * max_yaw_rate * dt, v], -1)


def step_forward_rel(state, out, ref_out):
    """The forward bar of the K1 tests (k1_check of tests/test_gpu_backward_float64.py explains it): the largest |out - ref_out| over
    max(|ref_out|, 1e-3, 0.05 x the row's largest operand), the operands being the old coordinates and the increments.  numpy float64 arrays."""
    operand = np.maximum(np.abs(state), np.abs(ref_out - state)).max(-1, keepdims=True)
    return float(np.max(np.abs(out - ref_out) / np.maximum(np.maximum(np.abs(ref_out), 1e-3), 0.05 * operand)))


def bicycle_step_model(state, action, lr, dt=0.1, max_acc=5.0, max_steer=math.pi / 2, left_handed=False, no_reversing=False):
    """KinematicBicycle.step / BicycleNoReversing.step as the reference writes them (kinematic.py:462-477, :513-523), in the dtype of the inputs:
    state (..., 4) [x, y, psi, v], action (..., 2) [acceleration, steering] normalised, lr (...).  The new speed drives the position along
    psi + beta and the heading through sin(beta) / lr; no_reversing replaces an acceleration that would make the speed negative by the one that
    stops the agent, -v / dt (the reference normalises and denormalises it on the way, and so does this)."""
    x, y, psi, v = state.unbind(-1)
    a, beta = action[..., 0] * max_acc, action[..., 1] * max_steer
    if no_reversing:
        a = torch.where(v + a * dt < 0, -v / dt, a)
        a, beta = (a / max_acc) * max_acc, (beta / max_steer) * max_steer
    if left_handed:
        beta = -beta
    v = v + a * dt
    return torch.stack([x + v * torch.cos(psi + beta) * dt, y + v * torch.sin(psi + beta) * dt, psi + (v / lr) * torch.sin(beta) * dt, v], -1)


def bicycle_clamp(state, action, dt=0.1, max_acc=5.0, **_):
    """-> (clamped, borderline), both (...,) bool, from float64: the rows whose acceleration BicycleNoReversing replaces (v + a dt < 0), and
    those within 1e-4 m/s of that switch -- a float32 evaluation may take either side there, and the two sides' gradients differ"""
    s, a = _t(state, F64), _t(action, F64)
    new = s[..., 3] + a[..., 0] * max_acc * dt
    return new < 0, new.abs() < 1e-4


def fit_action_model(future_xy, state, dt=0.1, max_acc=5.0, max_steer=math.pi / 2, left_handed=False):
    """KinematicBicycle.fit_action (kinematic.py:479-506): the normalised bicycle action that takes `state` (..., 4) to the position future_xy
    (..., 2) in one step of dt.  The steering is taken modulo 2 pi, and an agent that would have to turn by more than a right angle reverses."""
    x, y, psi, v = state.unbind(-1)
    vx, vy = (future_xy[..., 0] - x) / dt, (future_xy[..., 1] - y) / dt
    speed = torch.sqrt(vx ** 2 + vy ** 2)
    beta = torch.atan2(vy, vx) - psi * torch.sign(torch.abs(speed))
    beta = torch.remainder(beta + math.pi, 2 * math.pi) - math.pi
    reversing = torch.sign(torch.cos(beta)) == -1
    speed = speed * torch.where(reversing, -1.0, 1.0).to(speed.dtype)
    beta = torch.where(reversing, beta - math.pi * torch.sign(beta), beta)
    if left_handed:
        beta = -beta
    return torch.stack([((speed - v) / dt) / max_acc, beta / max_steer], -1)


def displacement_step_model(state, action, lr, max_dx=20.0, dt=0.1, oriented=False):
    """BicycleByDisplacement / BicycleByOrientedDisplacement.step (kinematic.py:526-587): the action (dx, dy) * max_dx (oriented: in the agent's own
    frame) names the position xy + (dx, dy) dt, fit_action_model turns it into a bicycle action and bicycle_step_model takes the step"""
    d = action * max_dx
    dx, dy = d[..., 0], d[..., 1]
    if oriented:
        c, s = torch.cos(state[..., 2]), torch.sin(state[..., 2])
        dx, dy = c * dx - s * dy, s * dx + c * dy
    target = torch.stack([state[..., 0] + dx * dt, state[..., 1] + dy * dt], -1)
    return bicycle_step_model(state, fit_action_model(target, state, dt=dt), lr, dt=dt)


#: the bicycle cases of the K1 tests: name -> keywords of _ops.bicycle_step and of bicycle_step_model alike
K1_BICYCLE_CASES = {
    'bicycle': dict(),
    'bicycle_lh': dict(left_handed=True),
    'bicycle_norev': dict(no_reversing=True),
    'bicycle_lh_norev_dt': dict(dt=0.25, max_acc=3.0, max_steer=0.9, left_handed=True, no_reversing=True),
}
K1_SIZES, K1_STRIDED = (1, 255, 256, 257, 1000), (300, 77)                # agent counts of the parametrised test; (n, seed) of the strided one


def k1_seed(n_action, n):
    return 1000 * n_action + n


def k1_inputs(n, n_action, seed, with_lr=False):
    """state as in test_k1_backward_matches_torch_autograd: x, y, psi in [-3, 3), v in [-1.2, 2.8); action in [-1, 1); the incoming gradient in
    [0, 1); lr in [1, 2), drawn last so that the other three do not depend on it.  With the speed on both sides of zero and |a dt| up to 0.5
    (0.75 in the dt case) about 30 % of the rows of a no-reversing case clamp."""
    gen = torch.Generator().manual_seed(seed)
    state = torch.cat([(torch.rand(n, 3, generator=gen) - 0.5) * 6, (torch.rand(n, 1, generator=gen) - 0.3) * 4], -1)
    action, wgt = (torch.rand(n, n_action, generator=gen) - 0.5) * 2, torch.rand(n, 4, generator=gen)
    return (state, action, wgt, 1 + torch.rand(n, generator=gen)) if with_lr else (state, action, wgt)
