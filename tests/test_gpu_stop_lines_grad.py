"""Differentiable stop-line observations on the device (csrc/stop_lines_bwd.hip `tds_stop_lines_bwd_f32`; _ops.stop_lines_grad) against the float64
torch-autograd model of their definition (tests/stop_lines_grad_model.py; include/tdship.h "K7b"), which is fed the very poses,
[sin, cos] and lines the kernels read, the index the forward wrote and the incoming gradient.

The bar is the project's own (tests/test_gpu_backward_float64.py):
    |kernel - float64 model| <= 4 x the largest |float32 model - float64 model| on the same inputs and tensor
-- the yardstick is computed here, from the model alone, and printed beside the kernel's figure (run with -s) before anything is asserted.  It holds
on ALL rows, with no exclusions: the model is fed the forward's own index.  Rows that must be zero are exactly zero.
Set TDS_STOP_LINES_GRAD_OUT=<file> to have the figures written as JSON (that is how profiles/stop_lines_grad_float64.json was made)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import lights_model as lm
import stop_lines_grad_model as gm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
F32 = np.float32
TENSORS = ('g_xy', 'g_sc')
#: (ahead_only, min_cos): both filters on, both off
FILTERS = ((True, 0.0), (False, None))


def record(label, figures):
    path = os.environ.get('TDS_STOP_LINES_GRAD_OUT')
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[label] = figures
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


def incoming(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def scene(seed, B, A, N):
    """lights_model.random_scenes -- duplicated line positions, absent agents and lines, observer 0 of every scene exactly on line N // 2 --, with
    that observer and its line present in scene 0; N = 0: no lines at all"""
    s = lm.random_scenes(seed, B, A, max(N, 1))
    s['agent_present'][0, 0] = True
    s['mask'][0, max(N, 1) // 2] = True
    s['agent_sc'][0, 0] = s['line_sc'][0, max(N, 1) // 2]               # heading along the line: it passes both filters (x = 0, cos_rel = 1)
    if N == 0:
        for key in ('lines', 'line_sc', 'mask', 'state', 'time_to_change'):
            s[key] = s[key][:, :0]
    return s


def run(s, k, reach, ahead_only, min_cos, g=None, seed=0, need=('agent_xy', 'agent_sc'), lines_require_grad=False):
    """forward and backward through _ops.stop_lines_grad from leaves of its own -> dict of numpy arrays: features, index, state, g, g_xy, g_sc (None
    for a leaf that did not require grad)"""
    from torchdrivesim_amd import _ops
    t = {key: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for key, v in s.items()}
    leaves = {key: t[key].clone().requires_grad_(key in need) for key in ('agent_xy', 'agent_sc')}
    lines = t['lines'].clone().requires_grad_(lines_require_grad)
    features, index, state = _ops.stop_lines_grad(leaves['agent_xy'], leaves['agent_sc'], t['agent_present'], lines, t['line_sc'], t['mask'], t['state'],
                                                  t['time_to_change'], k, reach, ahead_only=ahead_only, min_cos=min_cos)
    assert features.requires_grad == bool(need) and features.dtype == torch.float32
    for quiet in (index, state):
        assert not quiet.requires_grad and quiet.grad_fn is None and quiet.dtype == torch.int32
    g = incoming(features.shape, seed) if g is None else g
    if need:
        torch.autograd.backward([features], [g])
    assert lines.grad is None, 'the lines are constants'
    out = dict(features=features.detach().cpu().numpy(), index=index.cpu().numpy(), state=state.cpu().numpy(), g=g.cpu().numpy())
    for key, leaf in leaves.items():
        assert (leaf.grad is not None) == (key in need), key
        out['g_' + key[6:]] = None if leaf.grad is None else leaf.grad.cpu().numpy()
    return out


def hold(label, s, out, least=0):
    """every row of both gradient tensors against the model; each tensor's figure is printed before anything is asserted -> filled (B,A,K)"""
    args = (s['agent_xy'], s['agent_sc'], s['lines'], s['line_sc'], out['index'], out['g'])
    m64, m32 = gm.scene_gradients(*args), gm.scene_gradients(*args, torch.float32)
    filled = m64[2]
    seen = gm.observers(filled)
    failures, figures = [], {}
    for i, name in enumerate(TENSORS):
        got, w64, w32 = out[name].astype(np.float64), m64[i], m32[i]
        diff, yard, scale = float(np.abs(got - w64).max(initial=0.0)), float(np.abs(w32 - w64).max(initial=0.0)), float(np.abs(w64).max(initial=0.0))
        print(f'{label} {name}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}, filled slots {int(filled.sum())} of {filled.size}, observers with a line {int(seen.sum())} of {seen.size}')
        figures[name] = dict(kernel=diff, yardstick=yard, bound=FACTOR * yard, largest=scale)
        if not diff <= FACTOR * yard:
            failures.append(f'{label} {name}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not np.isfinite(got).all():
            failures.append(f'{label} {name}: not finite')
        if (got[~seen] != 0).any() or (w64[~seen] != 0).any():
            failures.append(f'{label} {name}: the row of an observer without a line is not exactly zero')
    figures['filled_slots'], figures['empty_slots'], figures['observers_without_a_line'] = int(filled.sum()), int((~filled).sum()), int((~seen).sum())
    record(label, figures)
    assert not failures, '\n'.join(failures)
    assert np.array_equal(filled, out['index'] >= 0) and filled.sum() >= least, (label, int(filled.sum()))
    return filled


def forward_bits_are_todays(s, k, reach, ahead_only, min_cos, out):
    want = lm.stop_lines(**s, k=k, max_distance=reach, ahead_only=ahead_only, min_cos=min_cos)
    for name, w in zip(('features', 'index', 'state'), want):
        assert np.array_equal(out[name].view(np.int32), w.view(np.int32)), name


# ------------------------------------------------------------------------------------------------------------------------ the bar
@pytest.mark.parametrize('N', [0, 1, 33, 65, 1024])
@pytest.mark.parametrize('A', [1, 5, 17, 65])
def test_random_scenes(A, N):
    """B = 2.  A: one observer, a part of a wave's 16 observers, a second wave with one observer, a second workgroup with one observer; N: no line, one,
    the boundaries of the forward's wave stride, the limit; K = 1, 4 and 32 (fewer slots than lanes, one each, eight each); both filters on and off; absent agents,
    duplicated line positions, and in scene 0 an observer exactly on a line's centre with a gradient on its distance"""
    s = scene(1000 * A + N, 2, A, N)
    filled_total = 0
    for K in (1, 4, 32):
        for ahead_only, min_cos in FILTERS:
            label = f'A={A} N={N} K={K} filters {"on" if ahead_only else "off"}'
            out = run(s, K, 60.0, ahead_only, min_cos, seed=A + N + K)
            forward_bits_are_todays(s, K, 60.0, ahead_only, min_cos, out)
            filled = hold(label, s, out)
            filled_total += int(filled.sum())
            absent = ~s['agent_present']
            assert not out['g_xy'][absent].any() and not out['g_sc'][absent].any() and not filled[absent].any()
            if N > 0:                   # the observer on the line: its nearest line is at distance exactly 0, with a gradient on the distance
                assert filled[0, 0, 0] and out['features'][0, 0, 0, 7] == 0 and out['g'][0, 0, 0, 7] != 0
                assert np.isfinite(out['g_xy'][0, 0]).all() and np.isfinite(out['g_sc'][0, 0]).all()
    assert (filled_total > 0) == (N > 0)
    if A == 65 and N >= 33:
        assert not s['agent_present'].all() and filled_total >= 200


def test_the_definition_cases():
    """lights_model.definition_cases(): the index by hand, every slot with a gradient of its own; the NaN pose and the absent observer get zeros"""
    c = lm.definition_cases()
    for (ahead_only, min_cos), index in lm.DEFINITION_INDEX.items():
        out = run(c, 4, lm.DEFINITION_MAX_DISTANCE, ahead_only, min_cos, seed=4)
        assert out['index'].tolist() == index
        forward_bits_are_todays(c, 4, lm.DEFINITION_MAX_DISTANCE, ahead_only, min_cos, out)
        hold(f'definition cases {ahead_only} {min_cos}', c, out, least=4)
        for key in TENSORS:
            assert not out[key][0, 2].any() and not out[key][1, 1].any(), key
        assert np.isfinite(out['g_xy'][1, 0]).all() and out['features'][1, 0, 0, 7] == 0, 'observer 0 of scene 1 stands on line 0'


# ------------------------------------------------------------------------------------------------------------------------ exact properties
def test_a_nan_at_an_empty_slot_changes_nothing_and_the_constants_feel_nothing():
    s = scene(65, 2, 17, 33)
    first = run(s, 32, 30.0, True, None, seed=5)
    empty = first['index'] < 0
    assert empty.sum() >= 100 and (~empty).sum() >= 40
    g = first['g'].copy()
    g[empty] = np.nan
    g[empty, 3] = np.inf
    g[empty, 7] = -np.inf
    g[~empty, 4:7] = np.nan                      # length, width, time_to_change: copies of constants, never read
    again = run(s, 32, 30.0, True, None, g=torch.from_numpy(g).to(DEV))
    for key in TENSORS:
        assert np.array_equal(first[key], again[key]) and np.isfinite(again[key]).all(), key
    hold('N33 with NaN at the empty slots', s, again)


def test_two_backward_runs_are_equal_and_subsets_of_the_inputs_work():
    s = scene(66, 2, 65, 65)
    first, again = run(s, 32, 60.0, False, None, seed=9), run(s, 32, 60.0, False, None, seed=9, lines_require_grad=True)
    for key in TENSORS:
        assert np.array_equal(first[key], again[key]) and np.abs(first[key]).max() > 0, key
    xy_only = run(s, 32, 60.0, False, None, seed=9, need=('agent_xy',))
    assert xy_only['g_sc'] is None and np.array_equal(xy_only['g_xy'], first['g_xy'])
    sc_only = run(s, 32, 60.0, False, None, seed=9, need=('agent_sc',))
    assert sc_only['g_xy'] is None and np.array_equal(sc_only['g_sc'], first['g_sc'])


def test_nothing_is_recorded_without_the_flag_grad_mode_or_a_leaf():
    from torchdrivesim_amd import _ops
    s = scene(67, 2, 5, 33)
    t = {key: torch.from_numpy(v).to(DEV) for key, v in s.items()}
    args = lambda xy: (xy, t['agent_sc'], t['agent_present'], t['lines'], t['line_sc'], t['mask'], t['state'], t['time_to_change'], 4, 60.0)
    leaf = t['agent_xy'].clone().requires_grad_(True)
    plain = _ops.stop_lines(*args(leaf))                                    # the plain form never records
    assert plain[0].grad_fn is None and not plain[0].requires_grad
    with torch.no_grad():
        quiet = _ops.stop_lines_grad(*args(leaf))
    assert quiet[0].grad_fn is None and not quiet[0].requires_grad
    nothing = _ops.stop_lines_grad(*args(t['agent_xy']))                    # nothing requires grad
    assert nothing[0].grad_fn is None and not nothing[0].requires_grad
    for other in (quiet, nothing):
        assert all(torch.equal(a, b) for a, b in zip(plain, other))
    live = _ops.stop_lines_grad(*args(leaf))
    assert live[0].grad_fn is not None and live[1].grad_fn is None and live[2].grad_fn is None and torch.equal(live[0].detach(), plain[0])


def test_garbage_in_the_index_is_never_dereferenced_and_outputs_are_written_in_full():
    """the entry point itself, with indices out of range and NaN incoming gradients there, into tensors that held NaN; then its argument rules"""
    from torchdrivesim_amd import _native as nat
    c = lm.definition_cases()
    t = {key: torch.from_numpy(v).to(DEV) for key, v in c.items()}
    index = torch.tensor(lm.DEFINITION_INDEX[(False, None)], dtype=torch.int32, device=DEV)
    index[0, 2] = torch.tensor([6, -7, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    index[1, 0] = torch.tensor([0, 1000000, 6, -1], dtype=torch.int32)
    g = incoming((2, 3, 4, 8), 8)
    bad = (index < 0) | (index >= 6)
    g[bad] = float('nan')
    outs = [torch.full((2, 3, 2), float('nan'), device=DEV) for _ in range(2)]
    dev = torch.device(DEV)
    nat.call('tds_stop_lines_bwd_f32', dev, t['agent_xy'], t['agent_sc'], t['lines'], t['line_sc'], index, g, *outs, 2, 3, 6, 4)
    got = dict(index=index.cpu().numpy(), g=g.cpu().numpy(), g_xy=outs[0].cpu().numpy(), g_sc=outs[1].cpu().numpy())
    args = (c['agent_xy'], c['agent_sc'], c['lines'], c['line_sc'], got['index'], got['g'])
    m64, m32 = gm.scene_gradients(*args), gm.scene_gradients(*args, torch.float32)
    assert not m64[2][0, 2].any() and m64[2][1, 0].tolist() == [True, False, False, False] and m64[2][0, 0].all()
    for i, key in enumerate(TENSORS):
        assert np.isfinite(got[key]).all(), key
        diff, yard = float(np.abs(got[key] - m64[i]).max()), float(np.abs(m32[i] - m64[i]).max())
        print(f'garbage {key}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g}')
        assert diff <= FACTOR * yard, key
        assert not got[key][0, 2].any() and not got[key][1, 1].any(), key
    # nothing to do: B * A == 0 is a successful no-op, and nothing is written
    nat.call('tds_stop_lines_bwd_f32', dev, None, None, None, None, None, None, None, None, 0, 3, 6, 4)
    nat.call('tds_stop_lines_bwd_f32', dev, None, None, None, None, None, None, None, None, 2, 0, 6, 4)
    # K7's rules and limits, refused before any launch: the outputs keep what they held
    outs = [torch.full((2, 3, 2), 7.0, device=DEV) for _ in range(2)]
    call = lambda N, K, gf=g: nat.call('tds_stop_lines_bwd_f32', dev, t['agent_xy'], t['agent_sc'], t['lines'], t['line_sc'], index, gf, *outs, 2, 3, N, K)
    for K in (0, 33, -1):
        with pytest.raises(nat.TdsError) as err:
            call(6, K)
        assert err.value.code == nat.E_INVAL
    with pytest.raises(nat.TdsError, match='LDS') as err:
        call(1025, 4)
    assert err.value.code == nat.E_LIMIT
    with pytest.raises(nat.TdsError, match='16 bytes') as err:
        call(6, 4, torch.zeros(2 * 3 * 4 * 8 + 1, device=DEV)[1:])
    assert err.value.code == nat.E_INVAL
    with pytest.raises(nat.TdsError, match='null') as err:
        nat.call('tds_stop_lines_bwd_f32', dev, t['agent_xy'], t['agent_sc'], t['lines'], t['line_sc'], None, g, *outs, 2, 3, 6, 4)
    with pytest.raises(RuntimeError, match='CPU'):
        nat.call('tds_stop_lines_bwd_f32', dev, t['agent_xy'].cpu(), t['agent_sc'], t['lines'], t['line_sc'], index, g, *outs, 2, 3, 6, 4)
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    # the host rules of the differentiable form are the forward's
    from torchdrivesim_amd import _ops
    for k, reach, min_cos in ((0, 10.0, None), (33, 10.0, None), (4, -1.0, None), (4, math.nan, None), (4, 10.0, math.nan)):
        with pytest.raises(ValueError):
            _ops.stop_lines_grad(t['agent_xy'].clone().requires_grad_(True), t['agent_sc'], t['agent_present'], t['lines'], t['line_sc'], t['mask'],
                                 t['state'], t['time_to_change'], k, reach, min_cos=min_cos)


def test_an_incoming_gradient_at_an_odd_offset_is_copied_not_refused():
    """_ops._aligned: a contiguous view whose data starts 4 bytes past a multiple of 16"""
    from torchdrivesim_amd import _ops
    s = scene(68, 2, 5, 33)
    base = run(s, 4, 60.0, False, None, seed=3)
    odd = torch.zeros(2 * 5 * 4 * 8 + 1, device=DEV)[1:].view(2, 5, 4, 8)
    odd.copy_(torch.from_numpy(base['g']).to(DEV))
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    again = run(s, 4, 60.0, False, None, g=odd)
    for key in TENSORS:
        assert np.array_equal(base[key], again[key]), key
