"""The differentiable route step on the device (csrc/route_bwd.hip `tds_route_progress_bwd_multi`; _ops.route_progress_grad;
RouteGoal(differentiable=True); Simulator) against the float64 torch-autograd model of its definition (tests/route_grad_model.py),
which is fed the very poses and [sin, cos] the kernels read, and the routes, cursors and stored progress the step found.

The bar is the project's own (tests/test_gpu_backward_float64.py):
    |kernel - float64 model| <= 4 x the largest |float32 model - float64 model| on the same inputs and tensor
-- the yardstick is computed here, from the model alone, and printed beside the kernel's figure (run with -s) before anything is asserted.  It
holds on ALL rows: the discrete choices are the forward's, which equal the model's bit for bit (tests/test_gpu_route_goals.py), so no row is
borderline.  Rows that must be zero (absent, without a route, a NaN pose) are exactly zero, and so are the state's columns past [x, y]."""
import numpy as np
import pytest
import torch

import route_grad_model as rgm
import route_model as rm
import test_gpu_route_goals as grg
from test_gpu_route_goals import DEV, pose_row, scene_states

pytestmark = pytest.mark.gpu
FACTOR = 4.0
FLOATS = rgm.FLOATS
F32 = np.float32


@pytest.fixture(scope='module')
def maps():
    """name -> (LaneletMap, model): Town01, the ring with its four segments a lanelet, with 122 (123 points: two turns of a wave's lanes) and with one"""
    import os
    from torchdrivesim_amd import lanelet2
    town = lanelet2.load_lanelet_map(os.path.join(grg.GOLDEN, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    out = {'town': (town, rm.Lanes(town))}
    for name, segments in (('ring', 4), ('ring122', 122), ('ring1', 1)):
        m = rm.ring_with_fork(segments=segments)
        out[name] = (m, rm.Lanes(m))
    return out


@pytest.fixture(scope='module')
def town02():
    import os
    from torchdrivesim_amd import lanelet2
    m = lanelet2.load_lanelet_map(os.path.join(grg.GOLDEN, 'carla_Town02.osm.gz'), origin=(0.0, 0.0))
    return m, rm.Lanes(m)


def routes_of(goal):
    """the routes and their state as the device holds them now, as the model's objects"""
    t = {k: goal._t[k].cpu().numpy() for k in ('lanes', 'n', 'start_arc', 'end_arc', 'offsets', 'length', 'cursor', 'stored')}
    B, A = t['n'].shape
    out = []
    for b in range(B):
        scene = []
        for a in range(A):
            n = int(t['n'][b, a])
            r = rm.Route(t['lanes'][b, a, :n].tolist(), float(t['start_arc'][b, a]), float(t['end_arc'][b, a]), [float(v) for v in t['offsets'][b, a, :n]],
                         float(t['length'][b, a]))
            r.cursor, r.stored = int(t['cursor'][b, a]), float(t['stored'][b, a])
            scene.append(r)
        out.append(scene)
    return out


def random_grads(goal, seed, names=FLOATS):
    """an incoming gradient for each named output (the others: none at all)"""
    B, A = goal.n.shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    shapes = dict(progress=(B, A), advance=(B, A), lateral=(B, A), heading=(B, A, 2), remaining=(B, A), lookahead=(B, A, goal.lookahead, 2))
    return {k: torch.randn(shapes[k], device=DEV, generator=g) for k in names}


def forward(goal, state, present=None):
    """one differentiable step from leaves of its own: -> (routes before the step, state leaf, [sin, cos] leaf, RouteProgress)"""
    from torchdrivesim_amd import _ops
    routes = routes_of(goal)
    st = state.clone().requires_grad_(True)
    sc = _ops.heading_sc(state[..., 2].detach().float()).requires_grad_(True)
    return routes, st, sc, goal.step(st, present, sc=sc)


def backward(out, grads, st, sc):
    terms = [(getattr(out, k) * g).sum() for k, g in grads.items() if g.numel() > 0]
    torch.autograd.backward(terms)
    zero = torch.zeros_like
    return (zero(st) if st.grad is None else st.grad).clone(), (zero(sc) if sc.grad is None else sc.grad).clone()


def hold(label, goal, models, routes, st, sc, present, grads, g_state, g_sc):
    """every row against the model; each tensor's figure is printed before anything is asserted.  -> the model's choices per row (None: no foot)"""
    B, A = goal.n.shape
    K, spacing = goal.lookahead, goal.spacing
    xy, scv = st.detach()[..., :2].float().cpu().numpy(), sc.detach().cpu().numpy()
    gn = {k: v.cpu().numpy() for k, v in grads.items()}
    got = dict(g_xy=g_state[..., :2].double().cpu().numpy(), g_sc=g_sc.double().cpu().numpy())
    g64, g32 = {k: np.zeros((B, A, 2)) for k in got}, {k: np.zeros((B, A, 2)) for k in got}
    found = np.zeros((B, A), bool)
    chosen = [[None] * A for _ in range(B)]
    for b in range(B):
        for a in range(A):
            here = True if present is None else bool(present[b, a])
            row = {k: v[b, a] for k, v in gn.items()}
            chosen[b][a] = rgm.choices(models[b], routes[b][a], xy[b, a, 0], xy[b, a, 1], scv[b, a, 0], scv[b, a, 1], K, spacing, here)
            found[b, a] = chosen[b][a] is not None
            for ref, dtype in ((g64, torch.float64), (g32, torch.float32)):
                ref['g_xy'][b, a], ref['g_sc'][b, a] = rgm.gradients(models[b], routes[b][a], xy[b, a], scv[b, a], row, K, spacing, here, dtype)
    failures = []
    for k in got:
        diff, yard, scale = float(np.abs(got[k] - g64[k]).max()), float(np.abs(g32[k] - g64[k]).max()), float(np.abs(g64[k]).max())
        print(f'{label} {k}: kernel against float64 {diff:.3g}, float32 model against float64 {yard:.3g} (bound {FACTOR * yard:.3g}), largest entry '
              f'{scale:.3g}, rows with a foot {int(found.sum())} of {found.size}')
        if not diff <= FACTOR * yard:
            failures.append(f'{label} {k}: {diff:.3g} > {FACTOR} x {yard:.3g}')
        if not np.isfinite(got[k]).all():
            failures.append(f'{label} {k}: not finite')
        if (got[k][~found] != 0).any() or (g64[k][~found] != 0).any():
            failures.append(f'{label} {k}: a row without a foot is not exactly zero')
    if bool((g_state[..., 2:] != 0).any()):
        failures.append(f'{label}: the state\'s columns past [x, y] are not zero')
    assert not failures, '\n'.join(failures)
    return chosen


def step_and_hold(label, goal, models, state, present=None, seed=1, names=FLOATS):
    grads = random_grads(goal, seed, names)
    routes, st, sc, out = forward(goal, state, present)
    g_state, g_sc = backward(out, grads, st, sc)
    assert g_state.shape == state.shape and g_sc.shape == state.shape[:2] + (2,)
    return hold(label, goal, models, routes, st, sc, None if present is None else present.cpu().numpy(), grads, g_state, g_sc), (g_state, g_sc)


def nudged(states, seed=0, amount=0.5):
    """the poses a little on from where the routes were dealt: beside the lane, turned, not on a centre line"""
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    return states + torch.cat([torch.rand(states.shape[:2] + (3,), device=DEV, generator=g) * amount, torch.zeros(states.shape[:2] + (1,), device=DEV)], -1)


# ------------------------------------------------------------------------------------------------------------------------ the bar
def test_the_ring_with_an_absent_row_a_row_without_a_route_and_a_nan_pose(maps):
    from torchdrivesim_amd.goals import RouteGoal
    ring_map, ring = maps['ring']
    states, present = grg.ring_batch(maps)
    goal = RouteGoal.sample(ring_map, states, present, seed=3, differentiable=True)
    assert goal.valid.cpu().tolist() == [[True, True, True], [True, False, False]], 'off the map, absent'
    moved = nudged(states)
    moved[0, 1, 0] = float('nan')
    chosen, _ = step_and_hold('ring', goal, [ring, ring], moved, present)
    assert [[c is not None for c in scene] for scene in chosen] == [[True, False, True], [True, False, False]]


@pytest.mark.parametrize('K', [0, 16, 32])
def test_town01_with_random_incoming_gradients_on_every_output(maps, K):
    """3 x 5 on Town01; twice from copies of the same goal: the two backward runs are bit-equal"""
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    states = grg.town_batch(maps)
    goal = RouteGoal.sample(town_map, states, seed=7, lookahead=K, spacing=4.0 if K < 32 else 2.5, differentiable=True)
    assert bool(goal.valid.all())
    twin = goal.copy()
    assert twin.differentiable
    moved = nudged(states, seed=K, amount=1.5)
    chosen, first = step_and_hold(f'Town01 K={K}', goal, [town] * 3, moved, seed=K)
    assert all(c is not None for scene in chosen for c in scene)
    assert len({(c['piece'], c['segment']) for scene in chosen for c in scene}) >= 5
    _, again = step_and_hold(f'Town01 K={K} (again)', twin, [town] * 3, moved, seed=K)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), 'the same inputs, the same bits'
    assert float(first[0].abs().max()) > 0 and float(first[1].abs().max()) > 0


def test_a_piece_wider_than_a_wave_and_a_piece_of_one_segment(maps):
    """lanelets of 123 centre-line points (122 segments: the lanes of a wave go round twice) and of two points (one segment)"""
    from torchdrivesim_amd.goals import RouteGoal
    for name in ('ring122', 'ring1'):
        ring_map, ring = maps[name]
        assert len(ring.cl[0]) == (123 if name == 'ring122' else 2)
        states = scene_states([[pose_row(ring, 0, 2.5), pose_row(ring, 1, 18.9, left=0.3), pose_row(ring, 3, 11.0, left=-0.5, turn=0.2)]])
        goal = RouteGoal.sample(ring_map, states, seed=5, length=30.0, lookahead=16, spacing=1.5, differentiable=True)
        assert bool(goal.valid.all())
        chosen, _ = step_and_hold(name, goal, [ring], nudged(states, amount=0.8))
        assert all(c is not None for c in chosen[0])
        if name == 'ring122':
            assert max(c['segment'] for c in chosen[0]) >= 64, 'a foot on the second turn of the lanes'


def test_feet_clamped_at_both_ends_of_a_route(maps):
    from torchdrivesim_amd.goals import RouteGoal
    ring_map, ring = maps['ring']
    start = scene_states([[pose_row(ring, 0, 2.5), pose_row(ring, 0, 2.5)]])
    goal = RouteGoal.sample(ring_map, start, seed=1, length=6.0, lookahead=8, spacing=1.0, differentiable=True)
    assert goal.length.cpu().tolist() == [[6.0, 6.0]] and goal.n.cpu().tolist() == [[1, 1]]
    poses = scene_states([[[1.0, 0.4, 0.3, 5.0], [9.75, -0.4, -0.2, 5.0]]])          # behind the start, beyond the end
    chosen, (g_state, _) = step_and_hold('clamped', goal, [ring], poses)
    assert [c['clamp'] for c in chosen[0]] == [-1, 1]
    assert float(g_state.abs().max()) > 0, 'lateral and the lookahead still move with the pose'


def test_some_incoming_gradients_absent(maps):
    """only lateral and lookahead take part in the loss: the other four incoming gradients reach the entry point as null pointers"""
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    states = grg.town_batch(maps, B=2, A=3)
    goal = RouteGoal.sample(town_map, states, seed=9, differentiable=True)
    step_and_hold('two of six', goal, [town] * 2, nudged(states), names=('lateral', 'lookahead'))
    step_and_hold('progress alone', goal, [town] * 2, nudged(states, seed=1), names=('progress',))


def test_alternating_town01_and_town02_scenes(maps, town02):
    """a wrong table pointer shows here: every other scene reads another lane table"""
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    two_map, two = town02
    models, lanelet_maps = [town, two, town, two], [town_map, two_map, town_map, two_map]
    rows = []
    for b, model in enumerate(models):
        ll = grg.long_lanelets(model, 4)
        rows.append([pose_row(model, ll[b], 4.0 + b, left=0.3), pose_row(model, ll[(b + 1) % 4], 6.5, left=-0.4, turn=0.1)])
    states = scene_states(rows)
    goal = RouteGoal.sample(lanelet_maps, states, seed=21, differentiable=True)
    assert bool(goal.valid.all())
    chosen, _ = step_and_hold('Town01 / Town02', goal, models, nudged(states))
    assert all(c is not None for scene in chosen for c in scene)


def test_a_state_of_three_columns_and_one_that_is_not_dense(maps):
    """xy_stride = 3, and a float64 state, which the launch reads from a dense float32 copy of [x, y]"""
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    states = grg.town_batch(maps, B=2, A=3)
    goal = RouteGoal.sample(town_map, states, seed=9, differentiable=True)
    twin = goal.copy()
    moved = nudged(states)
    _, (g3, s3) = step_and_hold('three columns', goal, [town] * 2, moved[..., :3].contiguous())
    wide = moved.double().requires_grad_(True)
    out = twin.step(wide)                                                   # [sin, cos] with torch inside: psi gets its gradient through them
    grads = random_grads(twin, 1)
    torch.autograd.backward([(getattr(out, k) * g).sum() for k, g in grads.items()])
    assert wide.grad.dtype == torch.float64 and not bool(wide.grad[..., 3].any())
    # (the float64 state's [sin, cos] are rounded to float32 for the launch: near, not equal, to torch's float32 sin / cos of the other run)
    torch.testing.assert_close(wide.grad[..., :2].float(), g3[..., :2], rtol=1e-4, atol=1e-3)
    sc = torch.stack([torch.sin(wide.detach()[..., 2]), torch.cos(wide.detach()[..., 2])], -1)
    torch.testing.assert_close(wide.grad[..., 2], (s3[..., 0].double() * sc[..., 1] - s3[..., 1].double() * sc[..., 0]), rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------------------------------ behaviour
def lap_goal(maps, **kw):
    from torchdrivesim_amd.goals import RouteGoal
    ring_map, ring = maps['ring']
    seed = grg.ring_seed(ring, [(0, 0, 0, 2.5), (0, 1, 3, 12.5)])
    states = scene_states([[pose_row(ring, 0, 2.5), pose_row(ring, 3, 12.5)]])
    return RouteGoal.sample(ring_map, states, seed=seed, **kw), ring, states


def test_backward_after_a_second_step_uses_the_first_steps_piece(maps):
    """row 0 stands before the joint of pieces 0 and 1 at the first step and beyond it at the second: the first step's backward, run after the
    second step, searches piece 0"""
    goal, ring, _ = lap_goal(maps, differentiable=True)
    first = scene_states([[pose_row(ring, 0, 18.0, left=0.3), pose_row(ring, 3, 14.0)]])
    second = scene_states([[pose_row(ring, 1, 3.0, left=0.3), pose_row(ring, 3, 17.0)]])
    grads = random_grads(goal, 2)
    routes, st, sc, out = forward(goal, first)
    assert goal.cursor.cpu().tolist() == [[0, 0]]
    kept = {k: getattr(out, k).clone() for k in FLOATS}
    later = goal.step(second.clone().requires_grad_(True))
    assert goal.cursor.cpu().tolist() == [[1, 0]], 'the cursor has moved on'
    assert all(torch.equal(getattr(out, k), kept[k]) for k in FLOATS), 'what a differentiable step returns outlives the next step'
    assert later.progress.data_ptr() != out.progress.data_ptr() and float(later.progress[0, 0].detach()) > float(out.progress[0, 0].detach())
    g_state, g_sc = backward(out, grads, st, sc)
    chosen = hold('after a second step', goal, [ring], routes, st, sc, None, grads, g_state, g_sc)
    assert chosen[0][0]['piece'] == 0


def test_backward_after_a_resample_raises(maps):
    goal, ring, states = lap_goal(maps, differentiable=True)
    _, st, sc, out = forward(goal, states)
    goal.resample(states)
    with pytest.raises(RuntimeError, match='dealt again'):
        out.progress.sum().backward()
    _, st, sc, out = forward(goal, states)                                  # a step on the new routes differentiates as ever
    out.progress.sum().backward()
    assert float(st.grad.abs().max()) > 0
    to = type(goal).to(maps['ring'][0], states, destination_lanes=torch.tensor([[2, 1]], dtype=torch.int32, device=DEV),
                       destination_arcs=torch.tensor([[5.0, 5.0]], dtype=torch.float64, device=DEV), differentiable=True)
    _, st, sc, out = forward(to, states)
    to.resample_to(states)
    with pytest.raises(RuntimeError, match='dealt again'):
        out.lateral.sum().backward()


def test_without_the_option_nothing_changes(maps):
    goal, ring, states = lap_goal(maps)
    assert goal.differentiable is False
    out = goal.step(states.clone().requires_grad_(True))
    t = goal._t
    assert all(getattr(out, k) is t[k] or getattr(out, k).data_ptr() == t[k].data_ptr() for k in FLOATS), 'the very buffers'
    assert all(getattr(out, k).grad_fn is None and not getattr(out, k).requires_grad for k in FLOATS)
    goal.differentiable = True
    with torch.no_grad():
        quiet = goal.step(states.clone().requires_grad_(True))
    assert quiet.progress.data_ptr() == t['progress'].data_ptr(), 'grad mode off: today\'s path'
    plain = goal.step(states)
    assert plain.progress.data_ptr() == t['progress'].data_ptr(), 'nothing requires grad: today\'s path'
    loud = goal.step(states.clone().requires_grad_(True))
    assert loud.progress.grad_fn is not None and loud.progress.data_ptr() != t['progress'].data_ptr()
    assert torch.equal(loud.progress, goal.last_progress.progress) and loud.reached.data_ptr() == t['reached'].data_ptr()
    for made in (goal.copy(), goal.copy().extend(2), goal.copy().select_batch_elements([0]), goal.copy().to(DEV)):
        assert made.differentiable


def sim_with_routes(maps, differentiable=True):
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    states = grg.town_batch(maps, B=2, A=3)
    goal = RouteGoal.sample([town_map] * 2, states, seed=31, differentiable=differentiable)
    return grg.make_sim([town_map] * 2, states, route_goals=goal), states


def route_loss(out):
    return -(out.advance.sum()) + (out.lateral ** 2).sum()


def test_through_the_simulator_equals_the_composition_by_hand(maps):
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.kinematic import KinematicBicycle
    sim, states = sim_with_routes(maps)
    twin = sim.route_goals.copy()
    action = torch.tensor([0.5, 0.05], device=DEV).expand(2, 3, 2).contiguous()
    a_sim = action.clone().requires_grad_(True)
    sim.step(a_sim)
    out = sim.compute_route_progress()
    assert out.advance.grad_fn is not None
    g_sim, = torch.autograd.grad(route_loss(out), a_sim)
    # by hand
    km = KinematicBicycle(dt=0.1)
    km.set_params(lr=torch.full((2, 3), 1.4, device=DEV))
    km.set_state(states.clone())
    a_hand = action.clone().requires_grad_(True)
    km.step(a_hand)
    st = km.get_state()
    f = _ops.route_progress_grad(twin._lane_table_set(), st, _ops.state_heading_sc(st), sim.present_mask, twin._t, twin._t, twin.goal_tolerance,
                                 twin.off_route_distance, twin.spacing)
    by_hand = dict(zip(_ops.ROUTE_FLOATS, f))
    assert all(torch.equal(by_hand[k], getattr(out, k)) for k in FLOATS)
    g_hand, = torch.autograd.grad(-(by_hand['advance'].sum()) + (by_hand['lateral'] ** 2).sum(), a_hand)
    assert torch.equal(g_sim, g_hand) and float(g_sim.abs().max()) > 0
    assert grg.same(grg.route_snapshot(sim.route_goals), grg.route_snapshot(twin))


def test_a_captured_forward_and_backward_replays_the_eager_ones(maps):
    """forward and backward of a step with a route loss in ONE HIP graph, on the single capture stream (tests/test_gpu_graph.py): three replays
    equal three eager steps of a twin bit for bit -- gradients, outputs and the routes' state"""
    sim, states = sim_with_routes(maps)
    ref, _ = sim_with_routes(maps)
    state = states.clone()
    action = torch.tensor([1.0, 0.1], device=DEV).expand(2, 3, 2).contiguous()

    def fwd_bwd(s, st, act):
        s.kinematic_model.set_state(st)
        s.step(act)
        out = s.compute_route_progress()
        g, = torch.autograd.grad(route_loss(out), act)
        return g, out.advance.detach(), s.get_state().detach()

    a_in = action.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd_bwd(sim, state, a_in)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        fwd_bwd(ref, state.clone(), action.clone().requires_grad_(True))
    torch.cuda.synchronize()
    assert grg.same(grg.route_snapshot(sim.route_goals), grg.route_snapshot(ref.route_goals))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = fwd_bwd(sim, state, a_in)
        state_next = got[2].clone()
    for i in range(3):
        want = fwd_bwd(ref, state.clone(), action.clone().requires_grad_(True))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(state_next, want[2]), i
        assert grg.same(grg.route_snapshot(sim.route_goals), grg.route_snapshot(ref.route_goals)), i
        assert float(want[0].abs().max()) > 0
        state.copy_(state_next)


def test_bad_arguments_are_refused_before_any_launch(maps):
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    goal, ring, states = lap_goal(maps)
    t = goal._t
    B, A = 1, 2
    sc = torch.zeros((B, A, 2), device=DEV)
    g_xy, g_sc = torch.zeros((B, A, 2), device=DEV), torch.zeros((B, A, 2), device=DEV)
    route = [t[name] for name, _, _ in _ops.ROUTE_TENSORS]

    def call(K=0, spacing=4.0, stride=4, out=g_xy):
        nat.call('tds_route_progress_bwd_multi', states.device, goal._lane_table_set().handle, None, B, A, states, stride, sc, None, *route, t['cursor'], None,
                 None, None, None, None, None, K, spacing, out, g_sc)

    call()
    for kw in (dict(K=33), dict(K=-1), dict(spacing=float('nan')), dict(spacing=-1.0), dict(stride=1), dict(out=None)):
        with pytest.raises(nat.TdsError) as e:
            call(**kw)
        assert e.value.code == nat.E_INVAL, kw
