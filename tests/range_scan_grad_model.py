"""
The yardstick of the range-scan backward (csrc/scan_bwd.hip, _ops.range_scan_grad; include/tdship.h "K5b").  Three things:

  forward64       a float64-INPUT restatement of the K5 definition (tests/range_scan_model.py rounds origins to float32; this one does not, so
                  that central differences can move an input by 1e-5), brute force over all faces and entities, with the model's own choices:
                  the entity, the slab, the exit edge and the chain of the fixed point (the gaps it bridged);
  scene_gradients the torch-autograd model of K5b in float64 (or float32, for the yardstick), GIVEN the choices (`choice`, `road_edge` -- the
                  kernel's witness or the model's own): t = (sigma h - l) / e of the binding slab, t = u_i + (u_j - u_i) w_i / (w_i - w_j) of
                  the edge;
  chain_state     the chain from (g_boxes, g_sc, g_ray_sc) to a state leaf [x, y, psi, v], psi through [sin, cos] of the entity and of its rays.

One scene per call of forward64; scene_gradients takes batches.
"""
import numpy as np
import torch

import range_scan_model as rm


# ------------------------------------------------------------------------------------------------------------------------ the forward, restated
def oriented(p, q):
    """an edge with its lexicographically (x, y) smaller end point first, as a 4-tuple"""
    p, q = (float(p[0]), float(p[1])), (float(q[0]), float(q[1]))
    return p + q if p <= q else q + p


def agent_choice(boxes, sc, present, a, d):
    """ray d = [dx, dy] of observer a against every other present rectangle, float64: (t0, entity or -1, slab 0 / 1 / 2) of the nearest entry,
    the lowest index on a tie -- K5's slab test in K5's order"""
    best = (np.inf, -1, 0)
    for j in range(len(boxes)):
        if j == a or not present[j]:
            continue
        rx, ry = boxes[a, 0] - boxes[j, 0], boxes[a, 1] - boxes[j, 1]
        s, c = sc[j]
        l = (rx * c + ry * s, ry * c - rx * s)
        e = (d[0] * c + d[1] * s, d[1] * c - d[0] * s)
        h = (boxes[j, 2] / 2, boxes[j, 3] / 2)
        t0, t1, ok, slab = 0.0, np.inf, True, 0
        for k in (0, 1):
            if e[k] == 0:
                ok = ok and abs(l[k]) <= h[k]
            else:
                u, v = (-h[k] - l[k]) / e[k], (h[k] - l[k]) / e[k]
                if min(u, v) > t0:
                    t0, slab = min(u, v), k + 1
                t1 = min(t1, max(u, v))
        if ok and t0 <= t1 and t0 < best[0]:
            best = (t0, j, slab)
    return best


def road_choice(tri, origin, d, max_range, gap):
    """R rays d (R, 2) from `origin` over the positive-area faces tri (F, 3, 2), all float64 -> per ray (road range, exit edge as an oriented
    4-tuple or None, the chain: the faces the fixed point reached over a gap, where gap_tolerance was used -- faces that share an edge follow
    each other without one, in an order that rounding decides and nothing depends on)"""
    origin, d = np.asarray(origin, np.float64), np.asarray(d, np.float64)
    r, f, a, b = rm.face_intervals(tri, origin, d, max_range, np.float64)
    out = []
    for k in range(len(d)):
        sel = np.nonzero(r == k)[0]
        F, chain = 0.0, []
        for i in sel[np.argsort(a[sel], kind='stable')]:
            if not a[i] <= F + gap:
                break
            if b[i] > F:
                if a[i] > F + 1e-9:                                      # reached over a real gap: the tolerance was used
                    chain.append(int(f[i]))
                F = b[i]
        F = min(F, float(max_range))
        edge = None
        if 0 < F < max_range:
            # the edges of the faces that end exactly there, by the tie rule: the smallest oriented 4-tuple
            cands = []
            for i in sel[b[sel] == F]:
                p = tri[f[i]] - origin
                w = d[k, 0] * p[:, 1] - d[k, 1] * p[:, 0]
                u = d[k, 0] * p[:, 0] + d[k, 1] * p[:, 1]
                for i0, i1 in ((0, 1), (1, 2), (2, 0)):
                    if w[i0] != w[i1] and min(w[i0], w[i1]) <= 0 <= max(w[i0], w[i1]) and u[i0] + (u[i1] - u[i0]) * (w[i0] / (w[i0] - w[i1])) == F:
                        cands.append(oriented(tri[f[i], i0], tri[f[i], i1]))
            edge = min(cands) if cands else None
        out.append((F, edge, tuple(chain)))
    return out


def near_faces(verts, faces, origin, reach):
    """(n, 3, 2) float64: the positive-area faces whose bounding box is within `reach` of origin"""
    verts, faces = np.asarray(verts, np.float32)[:, :2], np.asarray(faces, np.int64)
    tri = verts[faces[rm.positive_area(verts, faces)]].astype(np.float64)
    o = np.asarray(origin, np.float64)
    near = ((tri[..., 0].max(1) >= o[0] - reach) & (tri[..., 0].min(1) <= o[0] + reach) & (tri[..., 1].max(1) >= o[1] - reach) &
            (tri[..., 1].min(1) <= o[1] + reach))
    return tri[near]


def forward64(tri, boxes, sc, present, ray_sc, max_range, gap):
    """one scene, float64 inputs as they are: tri (F, 3, 2) positive-area faces or None, boxes (E, 5), sc (E, 2), present (E,), ray_sc (A, R, 2)
    -> dict(agents (A, R), road (A, R), choice (A, R, 2) int, edge [A][R] 4-tuple or None, chain [A][R])"""
    A, R = ray_sc.shape[:2]
    out = dict(agents=np.full((A, R), float(max_range)), road=np.full((A, R), float(max_range)), choice=np.zeros((A, R, 2), np.int64),
               edge=[[None] * R for _ in range(A)], chain=[[()] * R for _ in range(A)])
    out['choice'][..., 0] = -1
    for a in range(A):
        if not present[a]:
            continue
        d = np.asarray(ray_sc[a], np.float64)[:, ::-1]
        for k in range(R):
            t0, j, slab = agent_choice(boxes, sc, present, a, d[k])
            if t0 < max_range:
                out['agents'][a, k] = t0
                out['choice'][a, k] = (j, slab)
        if tri is not None and len(tri):
            for k, (F, edge, chain) in enumerate(road_choice(tri, boxes[a, :2], d, max_range, gap)):
                out['road'][a, k], out['edge'][a][k], out['chain'][a][k] = F, edge, chain
    return out


def edges_array(edge, A, R):
    """the model's exit edges as the witness states them: (A, R, 4) float64, NaN where there is none"""
    arr = np.full((A, R, 4), np.nan)
    for a in range(A):
        for k in range(R):
            if edge[a][k] is not None:
                arr[a, k] = edge[a][k]
    return arr


# ------------------------------------------------------------------------------------------------------------------------ the autograd model
def ranges_given_choices(boxes, sc, ray_sc, choice, road_edge):
    """torch, any dtype, batched: boxes (B, E, 5), sc (B, E, 2), ray_sc (B, A, R, 2), choice (B, A, R, 2) long, road_edge (B, A, R, 4) (NaN: none)
    -> (t_agent, live_agent, t_road, live_road), each (B, A, R): the differentiated expressions of K5b where the ray is live, 0 elsewhere"""
    B, A, R = ray_sc.shape[:3]
    who, slab = choice[..., 0], choice[..., 1]
    live_a = (who >= 0) & (slab > 0)
    j = who.clamp(min=0)
    bi = torch.arange(B, device=boxes.device)[:, None, None].expand(B, A, R)
    ent, esc = boxes[bi, j], sc[bi, j]                                     # B x A x R x 5 / 2
    obs = boxes[:, :A, None, :2]
    dx, dy = ray_sc[..., 1], ray_sc[..., 0]
    rx, ry = obs[..., 0] - ent[..., 0], obs[..., 1] - ent[..., 1]
    s, c = esc[..., 0], esc[..., 1]
    xs = slab == 1
    l = torch.where(xs, rx * c + ry * s, ry * c - rx * s)
    e = torch.where(xs, dx * c + dy * s, dy * c - dx * s)
    h = torch.where(xs, ent[..., 2], ent[..., 3]) / 2
    sigma = torch.where(e.detach() > 0, -torch.ones_like(e), torch.ones_like(e))
    e_safe = torch.where(live_a, e, torch.ones_like(e))
    t_agent = torch.where(live_a, (sigma * h - l) / e_safe, torch.zeros_like(e))
    live_r = torch.isfinite(road_edge).all(-1)
    ed = torch.where(live_r[..., None], road_edge, torch.zeros_like(road_edge)).to(boxes.dtype)
    pix, piy, pjx, pjy = ed[..., 0] - obs[..., 0], ed[..., 1] - obs[..., 1], ed[..., 2] - obs[..., 0], ed[..., 3] - obs[..., 1]
    ui, uj = dx * pix + dy * piy, dx * pjx + dy * pjy
    wi, wj = dx * piy - dy * pix, dx * pjy - dy * pjx
    D = torch.where(live_r, wi - wj, torch.ones_like(wi))
    t_road = torch.where(live_r, ui + (uj - ui) * (wi / D), torch.zeros_like(wi))
    return t_agent, live_a, t_road, live_r


def scene_gradients(boxes, sc, ray_sc, choice, road_edge, g_agent, g_road, dtype=torch.float64):
    """numpy in, numpy float64 out: (g_boxes (B, E, 5), g_sc (B, E, 2), g_ray_sc (B, A, R, 2), live_agent, live_road).  The inputs are cast to
    `dtype` first (float32: the yardstick).  g_agent / g_road None: that part is left out.  An incoming gradient at a dead ray is not read."""
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True)
    tb, ts, tr = t(boxes), t(sc), t(ray_sc)
    ch = torch.from_numpy(np.asarray(choice, np.int64))
    ed = torch.from_numpy(np.asarray(road_edge, np.float64))
    ta, la, trd, lr = ranges_given_choices(tb, ts, tr, ch, ed)
    loss = tb.sum() * 0 + ts.sum() * 0 + tr.sum() * 0
    if g_agent is not None:
        ga = torch.from_numpy(np.asarray(g_agent)).to(dtype)
        loss = loss + torch.where(la, ga * ta, torch.zeros_like(ta)).sum()
    if g_road is not None:
        gr = torch.from_numpy(np.asarray(g_road)).to(dtype)
        loss = loss + torch.where(lr, gr * trd, torch.zeros_like(trd)).sum()
    loss.backward()
    return (tb.grad.double().numpy(), ts.grad.double().numpy(), tr.grad.double().numpy(), la.numpy(), lr.numpy())


def touched(choice, live_agent, live_road, E):
    """(B, E) bool: entities some live ray ends on or whose own live ray observes"""
    B, A = choice.shape[:2]
    out = np.zeros((B, E), bool)
    b, a, k = np.nonzero(live_agent)
    out[b, choice[b, a, k, 0]] = True
    out[b, a] = True
    b, a, k = np.nonzero(live_road)
    out[b, a] = True
    return out


def chain_state(g_boxes, g_sc, g_ray_sc, sc, ray_sc, A, np_dtype=np.float64):
    """-> (B, A, 3) the gradient to [x, y, psi] of the exposed agents: psi through its own [sin, cos] node (d sin = cos, d cos = -sin, with the
    DEVICE's [sin, cos] values) and through [sin, cos] of each of its rays"""
    g_boxes, g_sc, g_ray_sc = (np.asarray(v, np_dtype) for v in (g_boxes, g_sc, g_ray_sc))
    sc, ray_sc = np.asarray(sc, np_dtype), np.asarray(ray_sc, np_dtype)
    psi = g_sc[:, :A, 0] * sc[:, :A, 1] - g_sc[:, :A, 1] * sc[:, :A, 0]
    psi = psi + (g_ray_sc[..., 0] * ray_sc[..., 1] - g_ray_sc[..., 1] * ray_sc[..., 0]).sum(-1)
    return np.stack([g_boxes[:, :A, 0], g_boxes[:, :A, 1], psi], -1).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------ scenes without a map
def random_boxes(seed, B, A, E, spread=None, absent=0.1):
    """B scenes of E rectangles scattered over a square (side grows with E so that rays meet a few), float32: dict(boxes, sc, present)"""
    g = np.random.default_rng(seed)
    spread = spread if spread is not None else 12.0 * np.sqrt(E)
    boxes = np.concatenate([g.uniform(-spread, spread, (B, E, 2)), g.uniform(3.0, 6.0, (B, E, 1)), g.uniform(1.5, 2.5, (B, E, 1)),
                            g.uniform(-np.pi, np.pi, (B, E, 1))], -1).astype(np.float32)
    sc = np.stack([np.sin(boxes[..., 4]), np.cos(boxes[..., 4])], -1).astype(np.float32)
    present = g.random((B, E)) >= absent
    present[:, 0] = True
    return dict(boxes=boxes, sc=sc, present=present)


def rays_of(boxes, A, R, fov=2 * np.pi):
    """(B, A, R, 2) float32 [sin, cos] of psi + off_k, off_k as Simulator.range_scan_angles states it"""
    k = np.arange(R, dtype=np.float64)
    off = (-fov / 2 + (fov * (k + 0.5)) / R).astype(np.float32)
    ang = boxes[:, :A, 4, None] + off
    return np.stack([np.sin(ang), np.cos(ang)], -1).astype(np.float32)
