"""The float64 autograd models of the backward kernels (tests/backward_models.py), CPU only: anchored to the reference's own autograd (fixture G7)
and to the oracle's forward values before they judge a kernel; the share of borderline rows of every input set the GPU tests use stays under its
cap; and the table the GPU tolerance comes from -- the same models in float32 against float64 -- is printed (run with -s to read it).

Printed here (largest |float32 model - float64 model| on the non-borderline rows, position / size / [sin, cos] gradient, beside the largest entry of
each): near the road 2.2e-5 / 1.1e-5 / 6.9e-5 of 41 / 8.8 / 47; around the edge of the lists' grid 0.023 / 0.010 / 0.054 of 704 / 122 / 1 135; 50 - 300 m
beyond the map 0.13 / 0.063 / 0.26 of 3 450 / 109 / 528 (short edges: the clamp term 2 (r . e) e / |e|^2 loses what r . e cancels); discs 4.1e-6 .. 2.8e-5 of
3.5 .. 21.

The bicycle step's model (bicycle_step_model, and fit_action_model for the displacement-driven bicycles) is anchored here too: to the reference's recorded
outputs (G1, G1b), to the oracle on the very inputs of the K1 GPU tests, and its no-reversing inputs are shown to use both branches."""
import functools

import numpy as np
import pytest
import torch

import backward_models as bm
from conftest import load_golden

THRESHOLDS = (0.5, 0.0, 25.0)
OFFROAD_CAP, DISCS_CAP = 0.02, 0.05          # largest share of borderline agents / boxes of an input set


@functools.lru_cache(maxsize=None)
def crop():
    return bm.town_crop()


@functools.lru_cache(maxsize=None)
def offroad_case(name, threshold):
    verts, faces = crop()
    inp = bm.offroad_inputs(name, verts)
    return inp, bm.offroad_reference(inp, bm.cpu_heading_sc(inp['state']), verts, faces, threshold)


@functools.lru_cache(maxsize=None)
def discs_case(name):
    inp = bm.discs_inputs(name)
    return inp, bm.discs_reference(inp)


# ------------------------------------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('metric', ['iou', 'discs'])
def test_offroad_model_reproduces_the_reference_autograd(metric):
    """G7: the reference's off-road loss of 2 x 6 agents and its torch-autograd gradient with respect to the state ([sin, cos] taken from psi
    inside).  Forward at the project's bar (rtol 1e-5); the gradient to 1e-5 of its largest entry (11.03: the float64 model differs from the
    recorded float32 autograd by 1.36e-5 absolute, the forward by 1.3e-5 at 15.5)."""
    g = load_golden('g7_grads.npz')
    s1 = g[f'{metric}_state1']
    inp = dict(state=s1, lenwid=g['size'], present=g['present'], grad_out=np.ones(s1.shape[:2], np.float32))
    r = bm.offroad_grads(inp, None, g['road_verts'], g['road_faces'], 0.5, sc_inside=True)
    np.testing.assert_allclose(r['loss'].numpy(), g[f'{metric}_off'], rtol=1e-5, atol=1e-5)
    ref = g[f'{metric}_grad_off_wrt_state1']
    diff = np.abs(r['gstate'].numpy() - ref).max()
    print(f'off-road model against G7 ({metric}): gradient {diff:.3g} of {np.abs(ref).max():.3g}')
    assert (np.abs(ref).max(-1) > 0).sum() >= 5 and diff <= 1e-5 * np.abs(ref).max()


def test_discs_model_reproduces_the_reference_autograd():
    """G7: the reference's discs collision of the same scenes and its gradient with respect to the state.  Forward to 2e-6 (the bar of
    test_gpu_backward.py); the gradient to 1e-5 of its largest entry (1.44: 2.7e-6 absolute here, the forward 1.5e-6)."""
    g = load_golden('g7_grads.npz')
    s1 = g['discs_state1']
    inp = dict(boxes=np.concatenate([s1[..., :2], g['size'], s1[..., 2:3]], -1), present=g['present'], n_exposed=None,
               grad_out=np.ones(s1.shape[:2], np.float32))
    out, gb = bm.discs_grads(inp)
    np.testing.assert_allclose(out.numpy(), g['discs_coll'], atol=2e-6)
    ref = g['discs_grad_coll_wrt_state1']
    got = np.concatenate([gb[..., :2].numpy(), gb[..., 4:5].numpy(), np.zeros(s1.shape[:2] + (1,))], -1)
    diff = np.abs(got - ref).max()
    print(f'discs model against G7: gradient {diff:.3g} of {np.abs(ref).max():.3g}')
    assert np.abs(ref).max() > 0 and diff <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize('name', bm.OFFROAD_SETS)
def test_offroad_model_forward_equals_the_oracle(oracle, name):
    """on the GPU tests' inputs, every threshold: the float64 model against the float32 restatement the forward kernels are pinned to"""
    verts, faces = crop()
    for thr in THRESHOLDS:
        inp, ref = offroad_case(name, thr)
        sc = bm.cpu_heading_sc(inp['state']).numpy()
        want = oracle.offroad(inp['state'], inp['lenwid'], verts, faces, thr, present=inp['present'], sc=sc)
        ok = ~ref['borderline'].numpy()                 # (a corner within rounding of the threshold may fall on either side of it)
        np.testing.assert_allclose(ref['g64']['loss'].numpy()[ok], want[ok], rtol=1e-5, atol=1e-5)
        assert (want > 0).any()


@pytest.mark.parametrize('name', list(bm.DISCS_SETS))
def test_discs_model_forward_equals_the_oracle(oracle, name):
    inp, ref = discs_case(name)
    want = oracle.collision(inp['boxes'], inp['present'], inp['n_exposed'], 'discs')
    ok = ~ref['borderline'].numpy()[:, :want.shape[1]]
    np.testing.assert_allclose(ref['out64'].numpy()[ok], want[ok], rtol=1e-5, atol=2e-6)
    assert (want > 0).sum() > 10


def test_discs_model_takes_the_heading_of_the_long_side():
    """two boxes end to end along x: a long one, and the same rectangle given as (width > length, psi - pi/2) -- the same discs, the same overlap,
    and a zero distance between two coinciding centres gives a finite gradient"""
    a = [0.0, 0.0, 4.0, 2.0, 0.3]
    for other in ([3.5, 1.0, 4.0, 2.0, 0.3], [3.5, 1.0, 2.0, 4.0, 0.3 - np.pi / 2]):
        inp = dict(boxes=np.array([[a, other, a]], np.float32), present=np.ones((1, 3), bool), n_exposed=None, grad_out=np.ones((1, 3), np.float32))
        out, g = bm.discs_grads(inp)
        assert torch.isfinite(g).all() and out[0, 1] > 0.1
        if other[2] > other[3]:
            first = out
        else:
            np.testing.assert_allclose(out.numpy(), first.numpy(), atol=1e-6)
            assert g[0, 1, 2].abs() > 0 and g[0, 1, 3].abs() > 0
    for dt in (bm.F32, bm.F64):                          # box 2 lies on box 0: distance 0 between their centres
        assert torch.isfinite(bm.discs_grads(inp, dt)[1]).all()


def test_step_models_against_hand_values():
    s = torch.tensor([[1.0, 2.0, 0.5, 3.0]], dtype=bm.F64)
    out = bm.unicycle_step_model(s, torch.tensor([[0.4, -0.2]], dtype=bm.F64), 0.1, 5.0, 1.0)[0]
    v = 3.0 + 0.4 * 5 * 0.1
    np.testing.assert_allclose(out.numpy(), [1 + v * np.cos(0.5) * 0.1, 2 + v * np.sin(0.5) * 0.1, 0.5 - 0.2 * 0.1, v], rtol=1e-12)
    a = torch.tensor([[0.1, -0.2, 0.3, 0.4]], dtype=bm.F64)
    np.testing.assert_allclose(bm.simple_step_model(s, a, 0.25, (2.0, 3.0, 4.0, 5.0))[0].numpy(),
                               [1 + 0.1 * 2 * 0.25, 2 - 0.2 * 3 * 0.25, 0.5 + 0.3 * 4 * 0.25, 3 + 0.4 * 5 * 0.25], rtol=1e-12)
    c, sn = np.cos(0.5), np.sin(0.5)
    np.testing.assert_allclose(bm.simple_step_model(s, a, 0.25, (2.0, 3.0, 4.0, 5.0), oriented=True)[0, :2].numpy(),
                               [1 + (c * 0.1 + sn * 0.2) * 2 * 0.25, 2 + (sn * 0.1 - c * 0.2) * 3 * 0.25], rtol=1e-12)
    g = load_golden('g1_kinematic.npz')                  # the reference's own outputs
    rel = lambda x, y: np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-3))
    s, a = torch.from_numpy(g['state']).to(bm.F64), torch.from_numpy(g['action4']).to(bm.F64)
    assert rel(bm.simple_step_model(s, a).numpy(), g['out_simple']) <= 1e-5
    assert rel(bm.simple_step_model(s, a, oriented=True).numpy(), g['out_oriented']) <= 1e-5


def rel_golden(x, y):
    """the bar tests/test_oracle_golden.py holds the oracle to"""
    return np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-3))


def test_bicycle_model_reproduces_the_reference_outputs():
    """G1: KinematicBicycle.step (plain, left-handed, dt = 0.25, two steps) and BicycleNoReversing.step as the reference computed them"""
    g = load_golden('g1_kinematic.npz')
    s, a, lr = (torch.from_numpy(g[k]).to(bm.F64) for k in ('state', 'action', 'lr'))
    for kw, key in ((dict(), 'out_bicycle'), (dict(left_handed=True), 'out_bicycle_lh'), (dict(dt=0.25), 'out_bicycle_dt'), (dict(no_reversing=True), 'out_norev')):
        assert rel_golden(bm.bicycle_step_model(s, a, lr, **kw).numpy(), g[key]) <= 1e-6, key
    two = bm.bicycle_step_model(bm.bicycle_step_model(s, a, lr), a.flip(0), lr)
    assert rel_golden(two.numpy(), g['out_bicycle_2steps']) <= 1e-6
    assert not np.array_equal(g['out_norev'], g['out_bicycle']), 'the fixture has rows that clamp'


def k1_bicycle_inputs():
    """(case, n, state, action, wgt, lr) of every bicycle case the GPU tests run: the parametrised agent counts and the strided one"""
    for name in bm.K1_BICYCLE_CASES:
        for n, seed in [(n, bm.k1_seed(2, n)) for n in bm.K1_SIZES] + [bm.K1_STRIDED]:
            yield (name, n) + bm.k1_inputs(n, 2, seed, with_lr=True)


def test_bicycle_model_equals_the_oracle_on_the_gpu_tests_inputs(oracle):
    """The model in the dtype of its inputs -- the float32 tensors of the K1 GPU tests, every case, agent count and the strided set -- against the float32
    restatement the forward kernel is pinned to, at the golden bar: 1e-6 of max(|value|, 1e-3).  Both are then float32 evaluations of the reference's
    expressions in the reference's order, clamped rows included, and differ in 1 - 26 of up to 4 000 coordinates by an ulp of sin / cos (measured: at most
    6.6e-7).  (Cast to float64 first the model cannot meet this bar, and no evaluation could: within 3 m of the origin many new coordinates are small
    differences of larger numbers, and the ORACLE's float32 rounding is 1.6e-5 .. 2.4e-5 of such a result, 1.2e-4 at a clamped row, where float32 leaves
    1.2e-7 and float64 0.  The test below measures that comparison in what float32 can keep; G1 holds the float64 model at this bar.)"""
    worst = 0.0
    for name, n, state, action, _, lr in k1_bicycle_inputs():
        kw = bm.K1_BICYCLE_CASES[name]
        assert state.dtype == action.dtype == lr.dtype == bm.F32
        want = oracle.bicycle_step(state.numpy(), action.numpy(), lr.numpy(), **kw)
        got = bm.bicycle_step_model(state, action, lr, **kw)
        assert got.dtype == bm.F32
        worst = max(worst, rel_golden(got.numpy(), want))
    print(f'bicycle model (float32, as its inputs) against the oracle on the K1 inputs: largest relative difference {worst:.3g}')
    assert worst <= 1e-6


def test_bicycle_model_equals_the_oracle_to_the_rounding_of_its_operands(oracle):
    """The FLOAT64 model against the oracle, the error measured in what float32 can keep: every new coordinate is old + increment, the increment a product of
    three or four rounded factors, so the oracle's result is within 4 float32 epsilons (2^-23) of the row's largest operand -- |old| or |increment| --
    of the exact value: half an epsilon for each of the sum, the products and sin / cos, with a factor two to spare.  A wrong term or sign in the
    model is 1e5 times that."""
    worst = 0.0
    for name, n, state, action, _, lr in k1_bicycle_inputs():
        kw = bm.K1_BICYCLE_CASES[name]
        want = oracle.bicycle_step(state.numpy(), action.numpy(), lr.numpy(), **kw)
        s = state.to(bm.F64)
        got = bm.bicycle_step_model(s, action.to(bm.F64), lr.to(bm.F64), **kw).numpy()
        operand = np.maximum(np.abs(s.numpy()), np.abs(got - s.numpy())).max(-1, keepdims=True)
        worst = max(worst, float(np.max(np.abs(want - got) / operand)) / 2.0 ** -23)
    print(f'bicycle model against the oracle on the K1 inputs: largest difference {worst:.3g} float32 epsilons of the row\'s largest operand')
    assert worst <= 4.0


def test_bicycle_no_reversing_inputs_use_both_branches_and_few_are_borderline():
    """from the float64 model alone, on the seeds of the GPU tests: 20 - 80 % of the rows clamp at every n >= 255, at most 1 % are within 1e-4 m/s of
    the switch; at a clamped row the model's gradient with respect to v and to the acceleration is zero (to 1e-12: (-v / dt) dt + v)"""
    seen = 0
    for name, n, state, action, wgt, lr in k1_bicycle_inputs():
        kw = bm.K1_BICYCLE_CASES[name]
        if not kw.get('no_reversing'):
            continue
        clamped, border = bm.bicycle_clamp(state, action, **kw)
        print(f'{name}, {n} agents: {int(clamped.sum())} rows clamp, {int(border.sum())} borderline')
        assert int(border.sum()) <= 0.01 * n
        if n >= 255:
            assert 0.2 * n <= int(clamped.sum()) <= 0.8 * n
        s, a, l = (t.to(bm.F64).requires_grad_(True) for t in (state, action, lr))
        (bm.bicycle_step_model(s, a, l, **kw) * wgt.to(bm.F64)).sum().backward()
        if bool(clamped.any()):
            assert float(s.grad[clamped][:, 3].abs().max()) <= 1e-12 and float(a.grad[clamped][:, 0].abs().max()) <= 1e-12
        free = ~clamped
        assert bool((s.grad[free][:, 3] != 0).all()) and bool((a.grad[free][:, 0] != 0).all())
        seen += int(clamped.sum())
    assert seen > 1000


def test_displacement_model_reproduces_the_reference_outputs():
    """G1b: fit_action_model then bicycle_step_model in float64 against BicycleByDisplacement / BicycleByOrientedDisplacement of the reference, and
    fit_action_model against the reference's fitted actions (G1), at the bars of tests/test_oracle_golden.py"""
    g = load_golden('g1b_bicycle_displacement.npz')
    s, a, lr = (torch.from_numpy(g[k]).to(bm.F64) for k in ('state', 'action', 'lr'))
    # the reference names the target x + dx dt in float32, at up to 290 m: half an ulp of x (3e-5 m) in each coordinate is 0.71 ulp / dt in the
    # fitted speed and, through the fitted steering (the arc v sin(beta) dt / lr, lr >= 1), less than one ulp in the new heading
    ulp_x = float(np.spacing(np.float32(np.abs(g['state'][..., :2]).max())))
    for name, kw in (('disp', {}), ('disp_max5', dict(max_dx=5.0, dt=0.2)), ('oriented', dict(oriented=True))):
        got, want = bm.displacement_step_model(s, a, lr, **kw).numpy(), g[f'out_{name}']
        assert rel_golden(got[..., :2], want[..., :2]) <= 1e-6, name
        assert np.abs(got[..., 3] - want[..., 3]).max() <= ulp_x / kw.get('dt', 0.1) and np.abs(got[..., 2] - want[..., 2]).max() <= ulp_x, name
    g = load_golden('g1_kinematic.npz')
    s, f = torch.from_numpy(g['state']).to(bm.F64), torch.from_numpy(g['future']).to(bm.F64)
    assert np.abs(bm.fit_action_model(f[..., :2], s).numpy() - g['fit_bicycle']).max() <= 1e-5
    assert np.abs(bm.fit_action_model(f[..., :2], s, left_handed=True).numpy() - g['fit_bicycle_lh']).max() <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ caps and yardsticks
@pytest.mark.parametrize('name', bm.OFFROAD_SETS)
def test_offroad_borderline_share_and_float32_yardstick(name):
    for thr in THRESHOLDS:
        inp, ref = offroad_case(name, thr)
        n = ref['borderline'].numel()
        share = int(ref['borderline'].sum()) / n
        scale = {k: float(ref['g64'][k].abs().max()) for k in bm.OFFROAD_GRADS}
        print(f'off-road {name} threshold {thr}: borderline {int(ref["borderline"].sum())} of {n}; float32 model against float64 '
              + ', '.join(f'{k} {ref["yard"][k]:.3g} of {scale[k]:.3g}' for k in bm.OFFROAD_GRADS))
        assert share <= OFFROAD_CAP
        assert all(torch.isfinite(ref['g32'][k]).all() and torch.isfinite(ref['g64'][k]).all() for k in bm.OFFROAD_GRADS)
        # rows without a gradient: exactly zero in the model too
        dead = torch.as_tensor(~inp['present'] | (inp['grad_out'] == 0))
        assert dead.sum() > 20 and all(bool((ref['g64'][k][dead] == 0).all()) for k in bm.OFFROAD_GRADS)
        # a yardstick is a float32 rounding figure: above zero, and small against the position gradient (the size and [sin, cos] gradients are
        # sums of the corners' with alternating signs, so they are judged against it too, as test_k2b_points_far_beyond_the_map does)
        for k in bm.OFFROAD_GRADS:
            assert 0 < ref['yard'][k] <= 2e-4 * scale['gstate']
    inp, ref = offroad_case(name, 0.5)
    if name == 'near':
        off = (ref['g64']['corners'] > 0.5).sum(-1)
        assert int(((off > 0) & (off < 4)).sum()) >= 20


@pytest.mark.parametrize('name', list(bm.DISCS_SETS))
def test_discs_borderline_share_and_float32_yardstick(name):
    inp, ref = discs_case(name)
    n = ref['borderline'].numel()
    scale = float(ref['g64'].abs().max())
    print(f'discs {name}: {bm.overlapping_pairs(inp)} overlapping pairs, borderline {int(ref["borderline"].sum())} of {n} boxes; float32 model against '
          f'float64 {ref["yard"]:.3g} of {scale:.3g}')
    assert int(ref['borderline'].sum()) / n <= DISCS_CAP
    assert torch.isfinite(ref['g32']).all() and 0 < ref['yard'] <= 2e-4 * scale
    wide = inp['boxes'][..., 3] > inp['boxes'][..., 2]
    assert 0.2 < wide.mean() < 0.4 and (ref['g64'][torch.as_tensor(wide)].abs().amax(-1) > 0).sum() > 10


def test_offroad_borderline_flags_a_corner_at_the_threshold():
    """a square road, one agent beside it: the flag is set where a corner's distance is within delta of sqrt(threshold), and not a metre away"""
    verts = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    for x, want in ((10.0 + 1.0 + np.sqrt(0.5) + 1e-3, True), (10.0 + 1.0 + np.sqrt(0.5) + 1.0, False), (5.0, False)):
        inp = dict(state=np.array([[[x, 5.0, 0.0, 0.0]]], np.float32), lenwid=np.array([[[2.0, 1.0]]], np.float32), present=np.ones((1, 1), bool),
                   grad_out=np.ones((1, 1), np.float32))
        flag = bm.offroad_borderline(inp, bm.cpu_heading_sc(inp['state']), verts, faces, 0.5)
        assert bool(flag[0, 0]) is want
    # 2 m to the right of the square with heading 0: the two near corners are 1 m out, the far ones 3 m; d(sum d^2)/dx = 2 (1 + 1 + 3 + 3)
    inp['state'][0, 0, 0] = 12.0
    r = bm.offroad_grads(inp, bm.cpu_heading_sc(inp['state']), verts, faces, 0.5)
    np.testing.assert_allclose(r['gstate'][0, 0].numpy(), [16.0, 0.0, 0.0, 0.0], atol=1e-9)
    np.testing.assert_allclose(r['glenwid'][0, 0].numpy(), [0.5 * 2 * (3 + 3 - 1 - 1), 0.0], atol=1e-9)
    np.testing.assert_allclose(r['loss'][0, 0].numpy(), 20.0, atol=1e-9)
