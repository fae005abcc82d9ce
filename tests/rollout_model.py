"""
The yardstick of a differentiable ROLLOUT: T simulator steps with a loss summed over the steps and one backward at the end -- the chain the project
exists for, which runs step to step through bicycle_step_bwd_kernel and the compact autograd nodes of simulator.py / _ops.py (the shared [sin, cos]
node, the boxes node, metrics foreseen on a side stream).  Plain torch, differentiated by torch autograd on the CPU, built from the models of
tests/backward_models.py (each anchored to the reference there):

    for t < T:   s = bicycle_step_model(s, actions[t], lr)
                 col_t = discs_collision_model([x, y, size, psi], present)
                 off_t = offroad_model(s, size, [sin psi, cos psi], verts, faces, threshold, present)
    loss = sum_t (col_t . wc[t] + off_t . wo[t])

Leaves: state0 (B, A, 4), actions (T, B, A, 2), lr (B, A), size (B, A, 2).  float64 is the reference, float32 the yardstick: what ANY float32 evaluation
of the chain may differ from float64 by.  tests/test_rollout_model.py holds the model to central differences of its own forward and caps the share of
borderline agents; tests/test_gpu_rollout.py holds the Simulator to 4 x the yardstick.

The weights are fixed and positive; about every 7th collision row and 10 % of the off-road rows have weight zero.  The collision value of an agent has no
`present` factor of its own (an absent agent still collects the overlaps of the present ones: Simulator.compute_collision), so the collision weights are
zero at absent agents as well -- a loss over the agents that exist -- and an absent agent's row of every gradient is then exactly zero.

With NPCs (n_npc > 0) the last n_npc agents of every scene are not stepped: their states are constants, the float32 roundings of the trajectory the
model computed for them as agents of its own -- what a ReplayController is given to replay -- and the leaves are the rows of the first A - n_npc agents.
"""
import functools

import numpy as np
import torch

import backward_models as bm
from backward_models import F32, F64, _t

GRADS = ('state0', 'actions', 'lr', 'size')
BORDERLINE_CAP = 0.10                    # largest share of borderline agents of a set
N_NPC = 8
COL_BAR, OFF_BAR = (1e-5, 2e-6), (1e-5, 1e-5)      # (rtol, atol) of test_discs_collision_gradient and of check_offroad, per step

#: name -> (B, A, T, seed, speeds (m/s), keywords of the bicycle step).  odd: 40 agents per scene are no multiple of the rows of a wavefront.
#: The seeds are chosen on the CPU, from the models alone (tests/test_rollout_model.py asserts both): at most BORDERLINE_CAP of the agents borderline,
#: and the float32 MODEL within the per-step bars of the metric values (COL_BAR, OFF_BAR) -- at coordinates of 100 m half an ulp of a disc centre, 4e-6 m
#: over r_i + r_j = 2 m and several pairs to a row, is of the size of the collision bar, and the float32 model itself misses it for about half of all seeds.
SETS = dict(plain=(3, 24, 4, 301, (2.0, 10.0), dict()),
            norev=(3, 24, 4, 302, (-0.2, 0.6), dict(no_reversing=True)),
            odd=(2, 40, 6, 353, (2.0, 10.0), dict()),
            four=(4, 16, 4, 304, (2.0, 10.0), dict()))


@functools.lru_cache(maxsize=None)
def crop():
    return bm.town_crop(bm.CROP_A)


def rollout_inputs(name):
    """The input sets, float32: every scene a cluster within +-7 m of a random vertex of the Town01 crop (agents on the road, across its edge and on each
    other), headings uniform, actions in [-1, 1] x [-0.3, 0.3], lr in [1, 2), 20 % of the boxes wider than long, about 10 % of the agents absent"""
    B, A, T, seed, (v0, v1), _ = SETS[name]
    verts = crop()[0]
    gen = np.random.default_rng(seed)
    xy = verts[gen.integers(0, len(verts), B)][:, None, :] + gen.uniform(-7.0, 7.0, (B, A, 2))
    state0 = np.concatenate([xy, gen.uniform(-np.pi, np.pi, (B, A, 1)), gen.uniform(v0, v1, (B, A, 1))], -1).astype(np.float32)
    actions = np.stack([gen.uniform(-1.0, 1.0, (T, B, A)), gen.uniform(-0.3, 0.3, (T, B, A))], -1).astype(np.float32)
    length, width = gen.uniform(4.0, 5.0, (B, A)), gen.uniform(1.8, 2.2, (B, A))
    wide = gen.random((B, A)) < 0.2
    size = np.stack([np.where(wide, width, length), np.where(wide, length, width)], -1).astype(np.float32)
    present = gen.random((B, A)) >= 0.1
    wc = gen.uniform(0.5, 1.5, (T, B, A)).astype(np.float32)
    wc[:, :, ::7] = 0.0
    wc *= present[None]
    wo = gen.uniform(0.5, 1.5, (T, B, A)).astype(np.float32)
    wo[gen.random((T, B, A)) < 0.1] = 0.0
    return dict(state0=state0, actions=actions, lr=gen.uniform(1.0, 2.0, (B, A)).astype(np.float32), size=size, present=present, wc=wc, wo=wo)


def rollout_grads(inp, verts, faces, dtype, T, metric='discs', threshold=0.5, *, npc_states=None, offroad=True, extra=None, forward_only=False, **bicycle_kw):
    """-> dict: the four gradients (float64 tensors, keys GRADS), `states` (T, B, A', 4), `col` and `off` (T, B, A'), `loss`: autograd of the chain in
    `dtype`.  npc_states (T, B, n, 4): the last n agents are NPCs at these states after each step (constants); A' = A - n, and so are the leaves' rows.
    offroad=False: the collision term alone.  extra(t, state_t) -> scalar: a further term of the loss (the route term of the route rollout).
    forward_only: no gradients, the loss and the per-step values alone (central differences)."""
    assert metric == 'discs'
    n = 0 if npc_states is None else npc_states.shape[2]
    E = inp['state0'].shape[1] - n
    leaves = dict(state0=_t(inp['state0'], dtype)[:, :E], actions=_t(inp['actions'], dtype)[:T, :, :E], lr=_t(inp['lr'], dtype)[:, :E],
                  size=_t(inp['size'], dtype)[:, :E])
    leaves = {k: v.clone().requires_grad_(not forward_only) for k, v in leaves.items()}
    present, wc, wo = np.asarray(inp['present']), _t(inp['wc'], dtype)[:, :, :E], _t(inp['wo'], dtype)[:, :, :E]
    all_size = torch.cat([leaves['size'], _t(inp['size'], dtype)[:, E:]], 1)
    s, loss, states, cols, offs = leaves['state0'], 0.0, [], [], []
    for t in range(T):
        s = bm.bicycle_step_model(s, leaves['actions'][t], leaves['lr'], **bicycle_kw)
        every = s if n == 0 else torch.cat([s, _t(npc_states[t], dtype)], 1)
        boxes = torch.cat([every[..., :2], all_size, every[..., 2:3]], -1)
        col = bm.discs_collision_model(boxes, present, E if n else None, dtype)
        loss = loss + (col * wc[t]).sum()
        cols.append(col.detach())
        if offroad:
            sc = torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1)
            off = bm.offroad_model(s, leaves['size'], sc, verts, faces, threshold, present[:, :E], dtype)
            loss = loss + (off * wo[t]).sum()
            offs.append(off.detach())
        if extra is not None:
            loss = loss + extra(t, s)
        states.append(s.detach())
    grads = [None] * 4 if forward_only else torch.autograd.grad(loss, [leaves[k] for k in GRADS], allow_unused=True)
    out = {k: (torch.zeros_like(leaves[k]) if g is None else g).to(F64) for k, g in zip(GRADS, grads)}
    out.update(states=torch.stack(states).to(F64), col=torch.stack(cols).to(F64), off=torch.stack(offs).to(F64) if offroad else None,
               loss=float(loss.detach()))
    return out


def rollout_borderline(inp, g64, verts, faces, T, threshold=0.5, *, npc_states=None, offroad=True, **bicycle_kw):
    """(B, A') bool, from the float64 model alone: the agents at which the loss is not differentiable within rounding at SOME step -- discs_borderline on
    that step's boxes, offroad_borderline (heading inside, unit weights) on that step's state, and for a no-reversing model a speed within 1e-4 m/s of the
    switch.  Such an agent is left out of all four comparisons, and of every step of `actions`."""
    n = 0 if npc_states is None else npc_states.shape[2]
    B, A = inp['present'].shape
    E = A - n
    present, size = np.asarray(inp['present']), _t(inp['size'], F64)
    flag = torch.zeros((B, E), dtype=torch.bool)
    before = _t(inp['state0'], F64)[:, :E]
    for t in range(T):
        s = g64['states'][t]
        every = s if n == 0 else torch.cat([s, _t(npc_states[t], F64)], 1)
        boxes = torch.cat([every[..., :2], size, every[..., 2:3]], -1)
        flag |= bm.discs_borderline(dict(boxes=boxes, present=present, n_exposed=E if n else None))[:, :E]
        if offroad:
            probe = dict(state=s, lenwid=size[:, :E], present=present[:, :E], grad_out=np.ones((B, E), np.float32))
            flag |= bm.offroad_borderline(probe, None, verts, faces, threshold, sc_inside=True)
        if bicycle_kw.get('no_reversing'):
            flag |= bm.bicycle_clamp(before, _t(inp['actions'], F64)[t, :, :E], **bicycle_kw)[1]
        before = s
    return flag


def values_at(inp, states, threshold=0.5, npc_states=None, offroad=True):
    """-> (col, off), each (T, B, A') float64: the float64 models of the two metrics AT the given per-step states (T, B, A', 4) -- the states the device
    reached, so that its metric values are judged on the very inputs its kernels read, as the single-step tests judge them.  (The chain's own float64
    states differ from the device's by the float32 rounding of a 100 m coordinate, 8e-6 m: that alone moves an off-road value of 2 d x 10 m by 1e-4.)"""
    verts, faces = crop()
    n = 0 if npc_states is None else npc_states.shape[2]
    E = states.shape[2]
    present, size = np.asarray(inp['present']), _t(inp['size'], F64)
    cols, offs = [], []
    with torch.no_grad():
        for t in range(states.shape[0]):
            s = _t(states[t], F64)
            every = s if n == 0 else torch.cat([s, _t(npc_states[t], F64)], 1)
            cols.append(bm.discs_collision_model(torch.cat([every[..., :2], size, every[..., 2:3]], -1), present, E if n else None, F64))
            if offroad:
                sc = torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1)
                offs.append(bm.offroad_model(s, size[:, :E], sc, verts, faces, threshold, present[:, :E], F64))
    return torch.stack(cols), torch.stack(offs) if offroad else None


def yardsticks(g64, g32, flag):
    """per gradient tensor the largest |float32 model - float64 model| over the agents that are not borderline"""
    ok = ~flag
    return {k: float((g32[k] - g64[k])[..., ok, :].abs().max()) if k in ('actions', 'size', 'state0') else float((g32[k] - g64[k])[ok].abs().max())
            for k in GRADS}


def reference_of(inp, T, npc_states=None, offroad=True, extra=None, **bicycle_kw):
    """What a rollout on the device is judged by: g64, g32 (rollout_grads in both dtypes), borderline (B, A') and yard"""
    verts, faces = crop()
    kw = dict(npc_states=npc_states, offroad=offroad, **bicycle_kw)
    g64 = rollout_grads(inp, verts, faces, F64, T, extra=extra, **kw)
    g32 = rollout_grads(inp, verts, faces, F32, T, extra=extra, **kw)
    flag = rollout_borderline(inp, g64, verts, faces, T, **kw)
    return dict(g64=g64, g32=g32, borderline=flag, yard=yardsticks(g64, g32, flag))


@functools.lru_cache(maxsize=None)
def reference(name, npc=False):
    """(inputs, reference) of a named set, computed once per process and never written to.  npc: the last N_NPC agents of every scene replay the float32
    roundings of their own trajectory in the set's plain reference; `npc_states` (T + 1, B, N_NPC, 4) float32, the initial state first, comes third."""
    B, A, T, _, _, kw = SETS[name]
    inp = rollout_inputs(name)
    if not npc:
        return inp, reference_of(inp, T, **kw)
    own = reference(name)[1]['g64']['states'][:, :, A - N_NPC:].to(F32)
    return inp, reference_of(inp, T, npc_states=own, **kw), torch.cat([_t(inp['state0'], F32)[None, :, A - N_NPC:], own])
