"""Float64 autograd model of the differentiable lane observations (include/tdship.h "K8b").

`choices` redoes the forward of tests/lane_obs_model.py for one observer with a GIVEN index, in float64 with that model's own functions (feet,
segment_foot, walk, point_at), and returns the discrete choices the definition names as constants of differentiation: per filled slot the foot's
segment sb and whether u was clamped, per point its validity, the lanelet its walk ends on and the segment there.  `observe64` is the same
forward without the rounding to float32: what the central differences of tests/test_lane_obs_grad_model.py are taken of.
`gradients` writes the eight features and the points of K8 in torch from those constants, in float64 or float32, and lets torch autograd
differentiate them.  It shares no code with the kernel's header csrc/tds_lane_obs_grad.h: the formulas of the backward are nowhere in this file."""
import math

import numpy as np
import torch

import lane_obs_model as lom

F32, F64 = np.float32, np.float64


def candidate(lanes, l, found):
    """whether index value l names a lanelet that is a candidate in K8's sense for the pose whose `feet` are `found`"""
    return lanes is not None and 0 <= l < len(lanes) and lom.usable(lanes, int(l)) and found[1][int(l)] >= 0


def choices(lanes, pose, index, n_points, spacing):
    """One observer.  pose (x, y, sin, cos) float32 values, index (k,) as K8 wrote it (or garbage) -> a list of k entries, None for a slot that
    is not filled, else a dict: l, sb, m (u unclamped and strictly inside (0, 1), l2 > 0), u (the clamped u, a constant where m is False), zero
    (distance == 0) and points: per point None (invalid) or (lanelet, segment, base) of the walk's end."""
    x, y, s, c = (float(F32(v)) for v in pose)
    out = [None] * len(index)
    if lanes is None or any(v != v for v in (x, y, s, c)):
        return out
    found = lom.feet(lanes, x, y)
    spacing = float(F32(spacing))
    for slot, l in enumerate(int(v) for v in index):
        if not candidate(lanes, l, found):
            continue
        sb = int(found[1][l])
        ax, ay, dx, dy, l2, u, fx, fy, dd = lom.segment_foot(lanes.cl[l], sb, x, y)
        with np.errstate(all='ignore'):
            u0 = ((x - ax) * dx + (y - ay) * dy) / l2 if l2 > 0 else 0.0
        cum = lanes.cum[l]
        arc = cum[sb] + u * (cum[sb + 1] - cum[sb])
        pts = []
        for j in range(n_points):
            q = arc + float(j) * spacing
            at = lom.walk(lanes, l, q)
            if at is None:
                pts.append(None)
                continue
            cur, base = l, 0.0                                   # the walk again, for the base it ends with (its validity is decided above)
            while q - base > lanes.length(cur):
                base, cur = base + lanes.length(cur), lanes.succ[cur][0]
            assert (cur, q - base) == at
            pts.append((cur, lom.point_at(lanes, cur, at[1])[2], base))
        out[slot] = dict(l=l, sb=sb, m=bool(l2 > 0 and 0.0 < u0 < 1.0), u=u, zero=dd == 0.0, points=pts)
    return out


def observe64(lanes, pose, k, n_points, spacing, max_distance):
    """lane_obs_model.observe without the rounding of its outputs, from the same functions: pose (x, y, sin, cos) float64 ->
    features (k, 8), points (k, n_points, 2) float64, index (k,), and `choices`-like keys (sb, m, per point (lanelet, segment) or None) to
    compare the discrete choices of two poses by"""
    x, y, s, c = (float(v) for v in pose)
    features, points = np.zeros((k, lom.FEATURES)), np.zeros((k, n_points, 2))
    index, keys = np.full(k, -1, np.int64), []
    d2, sb = lom.feet(lanes, x, y)
    spacing = float(F32(spacing))
    for slot, l in enumerate(lom.select(d2, sb, k, max_distance)):
        cl, cum = lanes.cl[l], lanes.cum[l]
        i = int(sb[l])
        ax, ay, dx, dy, l2, u, fx, fy, dd = lom.segment_foot(cl, i, x, y)
        u0 = ((x - ax) * dx + (y - ay) * dy) / l2 if l2 > 0 else 0.0
        ln = math.sqrt(l2)
        tx, ty = (dx / ln, dy / ln) if ln > 0 else (0.0, 0.0)
        arc = cum[i] + u * (cum[i + 1] - cum[i])
        features[slot] = [fx * c + fy * s, fy * c - fx * s, ty * c - tx * s, tx * c + ty * s, arc, cum[-1] - arc, tx * (y - ay) - ty * (x - ax),
                          math.sqrt(dd)]
        index[slot] = l
        key = [l, i, bool(l2 > 0 and 0.0 < u0 < 1.0)]
        for j in range(n_points):
            at = lom.walk(lanes, l, arc + float(j) * spacing)
            if at is None:
                key.append(None)
                continue
            wx, wy, seg, _ = lom.point_at(lanes, *at)
            ex, ey = wx - x, wy - y
            points[slot, j] = [ex * c + ey * s, ey * c - ex * s]
            key.append((at[0], seg))
        keys.append(tuple(key))
    return features, points, index, tuple(keys)


def constants(scene_lanes, xy, sc, index, n_points, spacing):
    """The discrete choices of a whole call as rows of constants: scene_lanes per scene a `Lanes` or None; xy, sc (B,A,2); index (B,A,K) ->
    filled (B,A,K) bool, valid (B,A,K,P) bool, S (n, 13) one row per filled slot, Q (n', 9) one row per valid point, both float64"""
    xy, sc, index = np.asarray(xy, F32), np.asarray(sc, F32), np.asarray(index)
    B, A, K = index.shape
    P = int(n_points)
    filled, valid = np.zeros((B, A, K), bool), np.zeros((B, A, K, P), bool)
    slots, pts = [], []
    for b in range(B):
        for a in range(A):
            lanes = scene_lanes[b]
            for k, ch in enumerate(choices(lanes, (xy[b, a, 0], xy[b, a, 1], sc[b, a, 0], sc[b, a, 1]), index[b, a], P, spacing)):
                if ch is None:
                    continue
                filled[b, a, k] = True
                l, sb = ch['l'], ch['sb']
                c0, c1, cum = lanes.cl[l][sb], lanes.cl[l][sb + 1], lanes.cum[l]
                sid = len(slots)
                slots.append((b, a, k, c0[0], c0[1], c1[0], c1[1], cum[sb], cum[sb + 1], cum[-1], float(ch['m']), ch['u'], float(ch['zero'])))
                for j, at in enumerate(ch['points']):
                    if at is None:
                        continue
                    valid[b, a, k, j] = True
                    cur, seg, base = at
                    p0, p1, cc = lanes.cl[cur][seg], lanes.cl[cur][seg + 1], lanes.cum[cur]
                    pts.append((sid, j, base, p0[0], p0[1], p1[0], p1[1], cc[seg], cc[seg + 1]))
    return filled, valid, np.array(slots, F64).reshape(-1, 13), np.array(pts, F64).reshape(-1, 9)


def observations(X, S, Q, spacing):
    """K8's features and points in torch, in the dtype of X: X (B,A,4) [x, y, sin, cos]; S, Q the rows of `constants` (S not empty) ->
    features (n, 8) of the filled slots, points (n', 2) of the valid points, and the (b, a, k) of the slots and (b, a, k, j) of the points"""
    dtype = X.dtype
    sb_, sa_, sk_ = (S[:, i].astype(np.int64) for i in range(3))
    t = lambda v: torch.as_tensor(np.asarray(v, F64)).to(dtype)
    x, y, s, c = X[sb_, sa_].unbind(-1)
    ax, ay, bx, by, cum0, cum1, last, m, uc, zero = (t(S[:, i]) for i in range(3, 13))
    m, zero = m > 0, zero > 0
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    safe = torch.where(l2 > 0, l2, torch.ones_like(l2))
    u = torch.where(m, ((x - ax) * dx + (y - ay) * dy) / safe, uc)
    ln = torch.sqrt(safe)
    tx, ty = torch.where(l2 > 0, dx / ln, torch.zeros_like(dx)), torch.where(l2 > 0, dy / ln, torch.zeros_like(dy))
    fx, fy = ax + u * dx - x, ay + u * dy - y
    dd = fx * fx + fy * fy
    zero = zero | (dd.detach() == 0)                          # (float32: a d2 that is above 0 in float64 may round to 0 here; the rule is the same)
    dist = torch.where(zero, torch.zeros_like(dd), torch.sqrt(torch.where(zero, torch.ones_like(dd), dd)))
    arc = cum0 + u * (cum1 - cum0)
    feats = torch.stack([fx * c + fy * s, fy * c - fx * s, ty * c - tx * s, tx * c + ty * s, arc, last - arc, tx * (y - ay) - ty * (x - ax), dist], -1)
    sid, j = Q[:, 0].astype(np.int64), Q[:, 1].astype(np.int64)
    base, px0, py0, px1, py1, k0, k1 = (t(Q[:, i]) for i in range(2, 9))
    pos = (arc[sid] + t(j) * float(F32(spacing))) - base
    w = k1 - k0
    tt = torch.where(w > 0, (pos - k0) / torch.where(w > 0, w, torch.ones_like(w)), torch.zeros_like(w))
    ex, ey = px0 + tt * (px1 - px0) - x[sid], py0 + tt * (py1 - py0) - y[sid]
    points = torch.stack([ex * c[sid] + ey * s[sid], ey * c[sid] - ex * s[sid]], -1)
    return feats, points, (sb_, sa_, sk_), (sb_[sid], sa_[sid], sk_[sid], j)


def gradients(scene_lanes, xy, sc, index, g_features, g_points, n_points, spacing, dtype=torch.float64):
    """The backward of a whole call by autograd: scene_lanes per scene a `Lanes` or None; xy, sc (B,A,2) float32 as the kernel read them; index
    (B,A,K) as it wrote it; g_features (B,A,K,8) and g_points (B,A,K,P,2) the incoming gradients, either None (zeros) -> g_xy, g_sc (B,A,2)
    float64 numpy, filled (B,A,K) bool, valid (B,A,K,P) bool.  The formula runs in `dtype` on the inputs widened (float64) or as they are
    (float32); the discrete choices are always those of the float64 forward.  What comes in at an empty slot or an invalid point is never read."""
    xy, sc = np.asarray(xy, F32), np.asarray(sc, F32)
    B, A = xy.shape[:2]
    filled, valid, S, Q = constants(scene_lanes, xy, sc, index, n_points, spacing)
    grad = np.zeros((B, A, 4))
    if len(S) and (g_features is not None or (g_points is not None and len(Q))):
        X = torch.tensor(np.concatenate([xy, sc], -1).astype(F64)).to(dtype).requires_grad_(True)
        feats, points, at_slots, at_points = observations(X, S, Q, spacing)
        loss = torch.zeros((), dtype=dtype)
        if g_features is not None:
            loss = loss + (feats * torch.as_tensor(np.asarray(g_features, F32)[at_slots]).to(dtype)).sum()
        if g_points is not None and len(Q):
            loss = loss + (points * torch.as_tensor(np.asarray(g_points, F32)[at_points]).to(dtype)).sum()
        loss.backward()
        grad = X.grad.double().numpy()
    return grad[..., :2].copy(), grad[..., 2:].copy(), filled, valid


def chain_state(g_xy, g_sc, sc, dtype=F64):
    """the gradient of the state [x, y, psi]: psi through [sin, cos] = the values `sc` the kernel read -> (B,A,3)"""
    s, c = np.asarray(sc)[..., 0].astype(dtype), np.asarray(sc)[..., 1].astype(dtype)
    gs, gc = g_sc[..., 0].astype(dtype), g_sc[..., 1].astype(dtype)
    return np.stack([g_xy[..., 0], g_xy[..., 1], (gs * c - gc * s).astype(F64)], -1)
