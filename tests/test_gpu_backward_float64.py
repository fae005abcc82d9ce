"""The hand-derived backward kernels against float64 torch-autograd models of their definitions (tests/backward_models.py; anchored to the
reference's own autograd and to the oracle in tests/test_backward_models.py).

    off-road   offroad_bwd_kernel through ops.offroad: all three gradients (state, size, [sin, cos] as leaves of their own), the three
               nearest-face searches (lists, hierarchy, grid rings), both entry points (one map, a map set), absent rows and rows without
               an incoming gradient, thresholds 0.5 / 0 / 25, agent counts that leave a wavefront half full
    discs      discs_pair_bwd under collision_scene_bwd_kernel (one chunk, several chunks, NPCs) and collision_bwd_kernel (rows)
    K1         simple_step (plain, oriented), unicycle_step, bicycle_step (plain, left-handed, no reversing; lr's gradient too): forward and backward

The bar, off-road and discs: on the rows the float64 model does not call borderline,
    |kernel - float64 model| <= 4 x the largest |float32 model - float64 model| on the same input set and tensor
-- the yardstick is computed here, from the model alone, and printed beside the kernel's figure (run with -s); the factor 4 is for another
order and contraction of the same float32 operations.  Borderline rows (at most 2 % of the agents, 5 % of the boxes: asserted on the CPU)
must be finite.  K1 is held to the project's own bars (see k1_check)."""
import functools

import numpy as np
import pytest
import torch

import backward_models as bm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0


@pytest.fixture(scope='module')
def ops():
    from torchdrivesim_amd import _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f64(t):
    return t.detach().cpu().to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------------- off-road
@functools.lru_cache(maxsize=None)
def crop(box=bm.CROP_A):
    return bm.town_crop(box)


@functools.lru_cache(maxsize=None)
def offroad_set(name):
    """(inputs, [sin, cos] as the device computes them -- what the kernel is given, so what the model is given)"""
    from torchdrivesim_amd import _ops
    inp = bm.offroad_inputs(name, crop()[0])
    return inp, _ops.heading_sc(dev(inp['state'])[..., 2]).cpu()


@functools.lru_cache(maxsize=None)
def offroad_ref(name, threshold, sc_inside=False):
    """computed once per (input set, threshold) and shared by the tests; never written to"""
    inp, sc = offroad_set(name)
    return bm.offroad_reference(inp, sc, *crop(), threshold, sc_inside=sc_inside)


def make_map(ops, box=bm.CROP_A):
    verts, faces = crop(box)
    return ops.StaticMap(verts, faces.astype(np.int32), device=DEV)


def run_offroad(ops, smap, inp, sc, threshold, rows=None):
    """-> loss and the three gradients of ops.offroad as float64 CPU tensors; rows: the first `rows` agents of the flattened set only"""
    pick = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(a.reshape((-1,) + a.shape[2:])[:rows]))
    state, lenwid = dev(pick(inp['state'])).requires_grad_(True), dev(pick(inp['lenwid'])).requires_grad_(True)
    scl = dev(pick(sc.numpy())).requires_grad_(True)
    out = ops.offroad(smap, state, lenwid, threshold=threshold, present=dev(pick(inp['present'])), sc=scl)
    out.backward(dev(pick(inp['grad_out'])))
    return dict(loss=f64(out), gstate=f64(state.grad), glenwid=f64(lenwid.grad), gsc=f64(scl.grad))


def hold(label, got, ref, keys=bm.OFFROAD_GRADS):
    """every tensor's figure is printed before anything is asserted"""
    ok = ~ref['borderline']
    failures = []
    for k in keys:
        assert got[k].shape == ref['g64'][k].shape
        diff = float((got[k] - ref['g64'][k])[ok].abs().max())
        yard, scale = ref['yard'][k], float(ref['g64'][k].abs().max())
        print(f'{label} {k}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}, borderline rows {int((~ok).sum())} of {ok.numel()}')
        if not diff <= FACTOR * yard:
            failures.append(f'{label} {k}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not bool(torch.isfinite(got[k]).all()):
            failures.append(f'{label} {k}: not finite')
    assert not failures, '\n'.join(failures)


def check_offroad(label, got, ref, inp):
    hold(label, got, ref)
    dead = torch.as_tensor(~inp['present'] | (inp['grad_out'] == 0))
    assert int(dead.sum()) > 20
    for k in bm.OFFROAD_GRADS:                                            # absent rows, rows without an incoming gradient: exactly zero
        assert bool((got[k][dead] == 0).all()), f'{label} {k}: a row without a gradient is not zero'
    assert bool((got['gstate'][..., 2:] == 0).all())                      # psi (its gradient flows through [sin, cos]) and the speed
    ok = ~ref['borderline']                                               # the forward kernel, on the way (pinned bit for bit elsewhere)
    np.testing.assert_allclose(got['loss'][ok].numpy(), ref['g64']['loss'][ok].numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('threshold', [0.5, 0.0, 25.0])
def test_offroad_near_the_road_edge(ops, threshold):
    """256 agents at crop vertices + N(0, 3 m): the candidate lists along a real road edge, agents half on the road"""
    inp, sc = offroad_set('near')
    ref = offroad_ref('near', threshold)
    got = run_offroad(ops, make_map(ops), inp, sc, threshold)
    check_offroad(f'off-road near, threshold {threshold}', got, ref, inp)
    nonzero = got['gstate'].abs().amax(-1) > 0
    off = (ref['g64']['corners'] > threshold).sum(-1)
    print(f'off-road near, threshold {threshold}: {int(nonzero.sum())} of {nonzero.numel()} agents with a gradient, '
          f'{int(((off > 0) & (off < 4)).sum())} with one to three corners off the road')
    assert bool((nonzero == (ref['g64']['gstate'].abs().amax(-1) > 0))[~ref['borderline']].all())
    assert int(((off > 0) & (off < 4) & nonzero).sum()) >= 5
    if threshold <= 0.5:                 # (5 m off the road -- threshold 25 -- are a few agents of this set, not a third of them)
        assert int(nonzero.sum()) * 3 >= nonzero.numel()


@pytest.mark.parametrize('name', ['edge', 'beyond'])
def test_offroad_around_and_beyond_the_lists_grid(ops, name):
    """edge: over the crop's bounding box +- 60 m -- the lists' grid ends 48 m out, so lists and hierarchy mix inside one wavefront;
    beyond: 50 - 300 m out, the hierarchy alone"""
    inp, sc = offroad_set(name)
    got = run_offroad(ops, make_map(ops), inp, sc, 0.5)
    check_offroad(f'off-road {name}', got, offroad_ref(name, 0.5), inp)
    assert int((got['gstate'].abs().amax(-1) > 0).sum()) * 2 >= got['loss'].numel()


@pytest.mark.parametrize('name', ['edge', 'beyond'])
def test_offroad_three_map_builds_against_the_model(ops, testing_lib, name):
    """1: lists + hierarchy; 2: lists, grid rings beyond them; 0: grid rings only -- each held to the model, not only to the others"""
    maps = {}
    for build in (1, 2, 0):
        testing_lib.tds_testing_set_near_lists(build)            # this hook exists only in libtdship_testing.so
        maps[build] = make_map(ops)
    testing_lib.tds_testing_set_near_lists(1)
    info = {b: m.info() for b, m in maps.items()}
    assert info[1]['near_candidates'] == info[2]['near_candidates'] > 0 and info[0]['near_candidates'] == 0 and info[1]['bytes'] > info[2]['bytes']
    inp, sc = offroad_set(name)
    ref = offroad_ref(name, 0.5)
    for build, label in ((1, 'lists + hierarchy'), (2, 'lists + rings'), (0, 'rings only')):
        check_offroad(f'off-road {name}, {label}', run_offroad(ops, maps[build], inp, sc, 0.5), ref, inp)


def test_offroad_agent_counts_that_leave_a_wavefront_half_full(ops):
    """n = 1, 3, 129 agents (32 lanes per agent, two agents per wavefront, eight per workgroup): the same bits as those rows of the full run"""
    inp, sc = offroad_set('near')
    smap = make_map(ops)
    full = run_offroad(ops, smap, inp, sc, 0.5)
    assert int((full['gstate'].abs().amax(-1) > 0).sum()) > 50
    for n in (1, 3, 129):
        part = run_offroad(ops, smap, inp, sc, 0.5, rows=n)
        for k in ('loss',) + bm.OFFROAD_GRADS:
            assert part[k].shape[0] == n and torch.equal(part[k], full[k].reshape((-1,) + full[k].shape[2:])[:n]), (n, k)


def test_offroad_map_set_equals_the_single_maps(ops):
    """tds_offroad_multi_bwd_f32: scenes 0 and 3 on the crop, 1 and 2 on a second crop ([80, 220] x [-10, 130], 8 115 faces) -- row for row the
    bits of the single-map runs (which the tests above hold to the model)"""
    ma, mb = make_map(ops), make_map(ops, bm.CROP_B)
    assert (ma.n_faces, mb.n_faces) == (4456, 8115)
    scene_map = [0, 1, 1, 0]
    mset = ops.StaticMapSet([ma, mb], torch.tensor(scene_map, dtype=torch.int32))
    for name in ('near', 'edge'):
        inp, sc = offroad_set(name)
        single = [run_offroad(ops, m, inp, sc, 0.5) for m in (ma, mb)]
        both = run_offroad(ops, mset, inp, sc, 0.5)
        for k in ('loss',) + bm.OFFROAD_GRADS:
            for b, w in enumerate(scene_map):
                assert torch.equal(both[k][b], single[w][k][b]), (name, k, b)
            assert not torch.equal(single[0][k], single[1][k])               # (the choice of the map matters on these inputs)
        assert all(int((both['gstate'][b].abs().amax(-1) > 0).sum()) > 10 for b in range(4))


def test_offroad_end_to_end_with_the_heading_inside(ops):
    """ops.offroad(m, state, lenwid) with sc=None: [sin, cos] taken from psi on the device, the psi column of the state gradient through them --
    against the model with sin / cos inside, under the same rule"""
    inp, _ = offroad_set('near')
    ref = offroad_ref('near', 0.5, True)
    state, lenwid = dev(inp['state']).requires_grad_(True), dev(inp['lenwid']).requires_grad_(True)
    out = ops.offroad(make_map(ops), state, lenwid, present=dev(inp['present']))
    out.backward(dev(inp['grad_out']))
    got = dict(gstate=f64(state.grad), glenwid=f64(lenwid.grad))
    hold('off-road near, end to end', got, ref, keys=('gstate', 'glenwid'))
    psi = got['gstate'][..., 2]
    print(f'off-road near, end to end: psi gradient, largest entry {float(psi.abs().max()):.3g}')
    assert int((psi != 0).sum()) * 3 >= psi.numel() and bool((got['gstate'][..., 3] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------- discs
@functools.lru_cache(maxsize=None)
def discs_case(name):
    inp = bm.discs_inputs(name)
    return inp, bm.discs_reference(inp)


#: input set -> (least number of overlapping pairs, least number of boxes with a gradient)
DISCS_FLOOR = dict(sparse=(200, 150), dense=(7000, 200), npc=(2000, 300), rows=(400, 200))


@pytest.mark.parametrize('name', list(bm.DISCS_SETS))
def test_discs_collision_gradient(ops, name):
    """sparse: 8 x 64 over 60 m (one chunk of the pair table); dense: 4 x 64 within 6 m (about 8 000 overlapping pairs: several chunks); npc:
    4 x 100 with 40 exposed; rows: 2 x 132, more than 16 384 pairs: one wavefront per row.  All five columns of the gradient with respect to
    the boxes -- the heading's through [sin, cos] of psi + pi/2 (width > length) -- against the model."""
    inp, ref = discs_case(name)
    B, N = inp['present'].shape
    A = N if inp['n_exposed'] is None else inp['n_exposed']
    assert (A * N > 16384) == (name == 'rows')
    boxes = dev(inp['boxes']).requires_grad_(True)
    out = ops.collision(boxes, dev(inp['present']), inp['n_exposed'], metric='discs')
    out.backward(dev(inp['grad_out']))
    got = f64(boxes.grad)
    ok = ~ref['borderline']
    diff = float((got - ref['g64'])[ok].abs().max())
    pairs, rows = bm.overlapping_pairs(inp), int((got.abs().amax(-1) > 0).sum())
    print(f'discs {name}: kernel against float64 {diff:.3g}, float32 model against float64 {ref["yard"]:.3g} (bound {FACTOR * ref["yard"]:.3g}), largest '
          f'entry {float(ref["g64"].abs().max()):.3g}; {pairs} overlapping pairs, {rows} of {B * N} boxes with a gradient, borderline {int((~ok).sum())}')
    assert pairs >= DISCS_FLOOR[name][0] and rows >= DISCS_FLOOR[name][1]
    assert bool(torch.isfinite(got).all())
    assert diff <= FACTOR * ref['yard']
    okf = ok[:, :A]
    np.testing.assert_allclose(f64(out)[okf].numpy(), ref['out64'][okf].numpy(), rtol=1e-5, atol=2e-6)
    wide = torch.as_tensor(inp['boxes'][..., 3] > inp['boxes'][..., 2])
    assert int((got[wide][:, 2:4].abs().amin(-1) > 0).sum()) > 10            # wide boxes with both size gradients: the heading + pi/2 branch
    if name == 'npc':
        assert int((got[:, A:].abs().amax(-1) > 0).sum()) > 100               # the NPC boxes receive gradients
    # a box that is absent and whose row has no incoming gradient takes part in nothing
    dead = torch.as_tensor(~inp['present'])
    dead[:, :A] &= torch.as_tensor(inp['grad_out'] == 0)
    assert bool((got[dead] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------- K1
NORM = (7.0, 3.0, 2.0, 1.5)
K1_CASES = {
    'simple': ('simple_step', 4, dict()),
    'oriented': ('simple_step', 4, dict(oriented=True)),
    'simple_norm_dt': ('simple_step', 4, dict(norm=NORM, dt=0.25)),
    'oriented_norm_dt': ('simple_step', 4, dict(norm=NORM, dt=0.25, oriented=True)),
    'unicycle': ('unicycle_step', 2, dict()),
    'unicycle_limits_dt': ('unicycle_step', 2, dict(dt=0.25, max_acc=3.0, max_yaw_rate=0.7)),
}
K1_CASES.update({name: ('bicycle_step', 2, kw) for name, kw in bm.K1_BICYCLE_CASES.items()})        # these carry lr, and its gradient


def has_lr(name):
    return K1_CASES[name][0] == 'bicycle_step'


def k1_inputs(n, n_action, seed, with_lr=False):
    """state as in test_k1_backward_matches_torch_autograd; with_lr: lr in [1, 2) as a fourth tensor"""
    return bm.k1_inputs(n, n_action, seed, with_lr)


def k1_model(name, state, action, wgt, lr=None):
    """-> (new state, gradient of the state, of the action[, of lr]) of the float64 model"""
    fn, _, kw = K1_CASES[name]
    leaves = [t.detach().to(torch.float64).requires_grad_(True) for t in (state, action) + (() if lr is None else (lr,))]
    out = getattr(bm, fn + '_model')(*leaves, **kw)
    (out * wgt.to(torch.float64)).sum().backward()
    return (out.detach(),) + tuple(t.grad for t in leaves)


def k1_check(label, state, out, gs, ga, ref, glr=None, borderline=None):
    """The project's bars.  Gradients: rtol 2e-4, atol 2e-5 (test_k1_backward_matches_torch_autograd), lr's too.  Forward: |kernel - model| <= 1e-5 of
    max(|model|, 1e-3) as in test_k1_bicycle_matches_oracle_and_golden -- where the new state is not a cancellation.  These states are a few
    metres from the origin and many of the 4 000 new coordinates are differences of two larger numbers; no float32 evaluation keeps 1e-5 of such a
    result (the float32 MODEL misses it by up to 1.2e-4 on these inputs), so the denominator is at least 0.05 x the row's largest operand: 1e-5 of
    it are 8 float32 epsilons of that operand (the float32 model stays within 4.4e-6 of this bar over 100 draws).
    borderline: rows at which the model's gradient is about to jump (bm.bicycle_clamp) -- left out of the gradient comparison, finite all the same;
    the forward is continuous there and is compared on every row."""
    ref_out, ref_gs, ref_ga = (t.numpy() for t in ref[:3])
    s = state.to(torch.float64).numpy()
    rel = bm.step_forward_rel(s, f64(out).numpy(), ref_out)
    ok = np.ones(len(s), bool) if borderline is None else ~borderline.numpy()
    pairs = [('state', f64(gs).numpy(), ref_gs), ('action', f64(ga).numpy(), ref_ga)] + ([] if glr is None else [('lr', f64(glr).numpy(), ref[3].numpy())])
    print(f'{label}: forward rel {rel:.3g} (bar 1e-5), gradient ' + ', '.join(f'of the {k} {np.abs(got - want)[ok].max():.3g} of {np.abs(want).max():.3g}'
                                                                            for k, got, want in pairs) +
          f' (bar rtol 2e-4, atol 2e-5), borderline rows {int((~ok).sum())} of {len(ok)}')
    assert rel <= 1e-5
    for k, got, want in pairs:
        assert got.shape == want.shape and np.isfinite(got).all(), k
        np.testing.assert_allclose(got[ok], want[ok], rtol=2e-4, atol=2e-5, err_msg=k)


def k1_check_clamp(name, state, action, gs, ga, n):
    """a no-reversing case: both branches at work (20 - 80 % of the rows clamp where n >= 255), and a clamped row passes nothing to its speed or its
    acceleration -- exactly zero.  -> the borderline rows, from the float64 model alone"""
    clamped, borderline = bm.bicycle_clamp(state, action, **K1_CASES[name][2])
    if n >= 255:
        assert 0.2 * n <= int(clamped.sum()) <= 0.8 * n
    stop = (clamped & ~borderline).to(gs.device)
    assert bool((gs[stop][:, 3] == 0).all()) and bool((ga[stop][:, 0] == 0).all())
    go = (~clamped & ~borderline).to(gs.device)
    assert bool((gs[go][:, 3] != 0).all()) and bool((ga[go][:, 0] != 0).all())
    return borderline


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
@pytest.mark.parametrize('name', list(K1_CASES))
def test_k1_step_forward_and_backward(ops, name, n):
    """agent counts around the workgroup size (KBLOCK = 256)"""
    fn, n_action, kw = K1_CASES[name]
    state, action, wgt, *lr = k1_inputs(n, n_action, bm.k1_seed(n_action, n), has_lr(name))
    s, a, *l = (t.to(DEV).requires_grad_(True) for t in [state, action] + lr)
    out = getattr(ops, fn)(s, a, *l, **kw)
    (out * wgt.to(DEV)).sum().backward()
    borderline = k1_check_clamp(name, state, action, s.grad, a.grad, n) if kw.get('no_reversing') else None
    k1_check(f'{name}, {n} agents', state, out, s.grad, a.grad, k1_model(name, state, action, wgt, *lr), *(t.grad for t in l), borderline=borderline)
    if kw.get('no_reversing'):
        assert float(s.grad[:, :3].abs().min()) > 0 and float(a.grad.abs().max()) > 0
    else:
        assert float(s.grad.abs().min()) > 0 and float(a.grad.abs().max()) > 0
    if l:
        assert float(l[0].grad.abs().max()) > 0


@pytest.mark.parametrize('name', ['oriented_norm_dt', 'unicycle_limits_dt'] + list(bm.K1_BICYCLE_CASES))
def test_k1_step_with_strided_views(ops, name):
    """state and action as transposed views, the incoming gradient as every other row of a larger tensor, lr as a column of a wider one"""
    fn, n_action, kw = K1_CASES[name]
    n, seed = bm.K1_STRIDED
    state, action, wgt, *lr = k1_inputs(n, n_action, seed, has_lr(name))
    s, a = state.t().contiguous().to(DEV).requires_grad_(True), action.t().contiguous().to(DEV).requires_grad_(True)
    l2 = [torch.stack([t, -t], -1).to(DEV).requires_grad_(True) for t in lr]                   # (n, 2): lr and a column that is not used
    lview = [t[:, 0] for t in l2]
    gout = torch.zeros(2 * n, 4)
    gout[::2] = wgt
    gview = gout.to(DEV)[::2]
    assert not s.t().is_contiguous() and not a.t().is_contiguous() and not gview.is_contiguous() and not any(t.is_contiguous() for t in lview)
    out = getattr(ops, fn)(s.t(), a.t(), *lview, **kw)
    out.backward(gview)
    borderline = k1_check_clamp(name, state, action, s.grad.t(), a.grad.t(), n) if kw.get('no_reversing') else None
    k1_check(f'{name}, strided views', state, out, s.grad.t(), a.grad.t(), k1_model(name, state, action, wgt, *lr), *(t.grad[:, 0] for t in l2),
             borderline=borderline)
    assert all(bool((t.grad[:, 1] == 0).all()) for t in l2)
