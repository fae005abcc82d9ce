"""The float64 model of a differentiable rollout (tests/rollout_model.py), CPU only, before it judges the Simulator (tests/test_gpu_rollout.py): its
gradient equals central differences of its own forward; every input set works both metrics (overlapping boxes, corners off the road) and all four
leaves; at most 10 % of the agents of a set are borderline; the float32 model meets the per-step bars of the metric values at its own states (the seeds
are chosen for these two, from the models alone); and the float32 yardsticks are printed (run with -s).

Printed here (largest |float32 model - float64 model| on the agents that are not borderline, state0 / actions / lr / size, beside the largest entry of
each): plain 2.0e-4 / 2.6e-4 / 2.6e-5 / 6.1e-5 of 139 / 88.5 / 12.1 / 43.3; norev 3.4e-4 / 1.7e-5 / 2.8e-6 / 1.2e-4 of 146 / 21.9 / 0.78 / 41.2; odd 1.6e-3 /
2.1e-3 / 3.0e-4 / 8.6e-5 of 419 / 536 / 76.4 / 82.1; four 3.3e-4 / 4.1e-4 / 1.8e-5 / 7.4e-5 of 231 / 304 / 29.8 / 25.9; 1 - 5 borderline agents of 48 - 80."""
import numpy as np
import pytest
import torch

import backward_models as bm
import rollout_model as rom

CASES = [(name, False) for name in rom.SETS] + [('plain', True)]


def case_id(case):
    return case[0] + ('-npc' if case[1] else '')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_borderline_share_entries_at_work_and_float32_yardstick(case):
    name, npc = case
    inp, ref = rom.reference(name, npc)[:2]
    g64, flag = ref['g64'], ref['borderline']
    B, E = flag.shape
    colliding, offroad = int((g64['col'] > 0).sum()), int((g64['off'] > 0).sum())
    print(f'rollout {case_id(case)}: borderline {int(flag.sum())} of {flag.numel()} agents; {colliding} colliding and {offroad} off-road (agent, step) entries of '
          f'{g64["col"].numel()}; float32 model against float64 ' + ', '.join(f'{k} {ref["yard"][k]:.3g} of {float(g64[k].abs().max()):.3g}' for k in rom.GRADS))
    assert int(flag.sum()) <= rom.BORDERLINE_CAP * flag.numel()
    assert colliding >= 50 and offroad >= 50
    for k in rom.GRADS:
        assert torch.isfinite(g64[k]).all() and torch.isfinite(ref['g32'][k]).all()
        assert int((g64[k] != 0).sum()) * 2 >= g64[k].numel(), f'{k}: fewer than half of the entries carry a gradient'
        # a yardstick is a float32 rounding figure: above zero, small against the tensor it belongs to
        assert 0 < ref['yard'][k] <= 1e-4 * float(g64[k].abs().max()), k
    # the per-step bars the device is held to are within reach of float32 on this set: the float32 model meets them at its own states
    npc_states = rom.reference(name, npc)[2][1:] if npc else None
    at32 = dict(zip(('col', 'off'), rom.values_at(inp, ref['g32']['states'].to(bm.F32), npc_states=npc_states)))
    for k, (rtol, atol) in (('col', rom.COL_BAR), ('off', rom.OFF_BAR)):
        diff, want = (ref['g32'][k] - at32[k])[:, ~flag].abs(), at32[k][:, ~flag].abs()
        print(f'rollout {case_id(case)}: float32 model\'s {k} against float64 at the same states {float(diff.max()):.3g}, nearest to its bar by '
              f'{float((atol + rtol * want - diff).min()):.3g}')
        assert bool((diff <= atol + rtol * want).all()), k
    absent = torch.as_tensor(~inp['present'][:, :E])
    assert int(absent.sum()) >= 2
    for k in rom.GRADS:                                             # an absent agent's rows: exactly zero in the model too
        assert bool((g64[k][..., absent, :] == 0).all() if g64[k].dim() > 2 else (g64[k][absent] == 0).all()), k
    if rom.SETS[name][5].get('no_reversing'):
        T = rom.SETS[name][2]
        before = torch.cat([torch.as_tensor(inp['state0'], dtype=bm.F64)[None], g64['states'][:-1]])
        clamped = bm.bicycle_clamp(before, inp['actions'][:T], **rom.SETS[name][5])[0]
        print(f'rollout {name}: {int(clamped.sum())} of {clamped.numel()} (agent, step) entries clamp')
        assert 0.2 * clamped.numel() <= int(clamped.sum()) <= 0.8 * clamped.numel()


@pytest.mark.parametrize('case', [('plain', False), ('norev', False)], ids=case_id)
def test_gradient_equals_central_differences_of_the_forward(case):
    """20 random coordinates of the four leaves, at agents that are not borderline: (loss(x + h) - loss(x - h)) / 2h in float64, h = 1e-6, against the
    autograd gradient within 1e-6 of the largest entry of that leaf's gradient (the loss is a sum of hundreds of squared distances of a few metres: its
    float64 rounding over 2h is 1e-8, the third derivative's term h^2 f''' / 6 less still; a kink within h of an agent would show, which is what the
    borderline flag -- 1e-4 and 2e-3 wide -- is there to exclude)"""
    name, npc = case
    B, A, T, seed, _, kw = rom.SETS[name]
    out = rom.reference(name, npc)
    inp, ref, npc_states = out[0], out[1], (out[2][1:] if npc else None)
    verts, faces = rom.crop()
    gen = np.random.default_rng(seed + 1000)
    ok = np.argwhere(~ref['borderline'].numpy() & inp['present'][:, :ref['borderline'].shape[1]])
    h, worst = 1e-6, 0.0
    for i in range(20):
        k = rom.GRADS[i % 4]
        b, a = ok[gen.integers(len(ok))]
        index = dict(state0=(b, a, gen.integers(4)), actions=(gen.integers(T), b, a, gen.integers(2)), lr=(b, a), size=(b, a, gen.integers(2)))[k]
        index = tuple(int(v) for v in index)
        losses = []
        for sign in (1.0, -1.0):
            moved = dict(inp)
            moved[k] = np.asarray(inp[k], np.float64).copy()
            moved[k][index] += sign * h
            losses.append(rom.rollout_grads(moved, verts, faces, bm.F64, T, npc_states=npc_states, forward_only=True, **kw)['loss'])
        fd, an = (losses[0] - losses[1]) / (2 * h), float(ref['g64'][k][index])
        scale = float(ref['g64'][k].abs().max())
        worst = max(worst, abs(fd - an) / scale)
        assert abs(fd - an) <= 1e-6 * scale, (k, index, fd, an, scale)
    print(f'rollout {case_id(case)}: central differences against autograd, largest difference {worst:.3g} of the leaf\'s largest entry')
