"""Route goals on the device (csrc/route.hip `tds_route_sample_multi`, `tds_route_progress_multi`, `tds_route_points_multi`; goals.RouteGoal;
Simulator(route_goals=...)) against the float64 model of their definition (tests/route_model.py), which is fed the very poses -- [sin, cos]
included, computed on the device with torch.sin / torch.cos -- the kernels read.

The bar: lanes, n, cursor and the flags equal; arcs, offsets, lengths and every float output equal BIT FOR BIT (the kernels are float64
+ - * / sqrt built with -ffp-contract=off, the model the same expressions in the same order).  No row is excepted."""
import math
import os

import numpy as np
import pytest
import torch

import lane_follow_model as lf
import route_model as rm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
FLOATS = ('progress', 'advance', 'lateral', 'heading', 'remaining', 'lookahead')


@pytest.fixture(scope='module')
def maps():
    """name -> (LaneletMap, model)"""
    from torchdrivesim_amd import lanelet2
    town = lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    ring = rm.ring_with_fork()
    return {'town': (town, rm.Lanes(town)), 'ring': (ring, rm.Lanes(ring))}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def pose_row(model, lanelet, arc, left=0.0, turn=0.0):
    """[x, y, psi, speed] on a centre line, optionally `left` metres beside it and turned by `turn`"""
    x, y, psi, sn, cs = (float(v) for v in model.pose(lanelet, arc))
    return [x - left * sn, y + left * cs, psi + turn, 5.0]


def long_lanelets(model, n):
    ok = [l for l in range(len(model)) if model.eligible(l) and not model.flag[l]]
    return sorted(ok, key=lambda l: -model.length(l))[:n]


def ring_seed(model, rows, start=0):
    """a seed with which every (scene id, agent, lanelet, arc) of `rows` gets its full 200 m on the ring (never draws the fork's dead end)"""
    for seed in range(start, start + 100000):
        if all(rm.sample(model, l, arc, 200.0, seed, s, a).length == 200.0 for s, a, l, arc in rows):
            return seed
    raise AssertionError('no such seed')


def model_routes(goal, models, states, present=None, rows=None):
    """the model's route of every row, from the snap the model makes of the poses and the [sin, cos] the device computed for them"""
    xy, sc = states[..., :2].cpu().numpy().astype(F32), goal._t['sc'].cpu().numpy()
    D, ids = goal.requested_length.cpu().numpy(), goal.scene_ids.cpu().numpy()
    B, A = xy.shape[:2]
    out = [[None] * A for _ in range(B)]
    for b in range(B):
        for a in range(A):
            if rows is not None and not rows[b][a]:
                continue
            if models[b] is None:
                out[b][a] = rm.Route()
                continue
            lane, arc, _ = lf.snap(models[b], xy[b, a, 0], xy[b, a, 1], sc[b, a, 0], sc[b, a, 1], goal.tolerance)
            out[b][a] = rm.sample(models[b], lane, arc, D[b, a], goal.seed, int(ids[b]), a, True if present is None else bool(present[b][a]))
    return out


def assert_routes(goal, routes, what=''):
    t = {k: goal._t[k].cpu().numpy() for k in ('lanes', 'n', 'start_arc', 'end_arc', 'offsets', 'length', 'cursor', 'stored', 'completed')}
    for b, scene in enumerate(routes):
        for a, r in enumerate(scene):
            if r is None:
                continue
            tag = (what, b, a)
            assert t['n'][b, a] == r.n, (tag, t['n'][b, a], r.n)
            assert t['lanes'][b, a].tolist() == r.lanes + [-1] * (16 - r.n), (tag, t['lanes'][b, a], r.lanes)
            assert bits(t['offsets'][b, a]) == bits(np.array(r.offsets + [0.0] * (16 - r.n))), (tag, t['offsets'][b, a], r.offsets)
            for k, v in (('start_arc', r.start_arc), ('end_arc', r.end_arc), ('length', r.length), ('stored', r.stored)):
                assert bits(t[k][b, a]) == bits(np.float64(v)), (tag, k, t[k][b, a], v)
            assert t['cursor'][b, a] == r.cursor and bool(t['completed'][b, a]) == r.completed, tag


def step_and_compare(goal, models, routes, states, present=None, what=''):
    """one RouteGoal.step; every output of every row against the model (which moves its routes' cursors on as the kernel does)"""
    out = goal.step(states, present)
    got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
    xy, sc = states[..., :2].cpu().numpy().astype(F32), goal._t['sc'].cpu().numpy()
    K = goal.lookahead
    for b, scene in enumerate(routes):
        for a, r in enumerate(scene):
            want = rm.progress(models[b], r, xy[b, a, 0], xy[b, a, 1], sc[b, a, 0], sc[b, a, 1], goal.goal_tolerance, goal.off_route_distance, K,
                               goal.spacing, True if present is None else bool(present[b, a]))
            tag = (what, b, a)
            for k in FLOATS:
                assert bits(got[k][b, a]) == bits(np.asarray(want[k], F32)), (tag, k, got[k][b, a], want[k])
            assert bool(got['reached'][b, a]) == want['reached'] and bool(got['off_route'][b, a]) == want['off_route'], tag
    assert_routes(goal, routes, what)
    return got


def scene_states(rows):
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- sampling
def ring_batch(maps):
    """B = 2 x A = 3 on the ring: mid-lanelet poses, one beside its lane and turned a little, one absent, one off the map"""
    _, ring = maps['ring']
    states = scene_states([[pose_row(ring, 0, 2.5), pose_row(ring, 2, 7.0, left=0.4, turn=0.1), pose_row(ring, 4, 3.0)],
                           [pose_row(ring, 3, 12.5), [500.0, 500.0, 0.3, 1.0], pose_row(ring, 1, 9.0, left=-0.3)]])
    present = torch.tensor([[True, True, True], [True, True, False]], device=DEV)
    return states, present


def town_batch(maps, B=3, A=5):
    """B x A on Town01, poses on the longest lanelets and in junctions (the lanelets that follow them), none closer than 3 m to a lanelet's end"""
    _, town = maps['town']
    ll = long_lanelets(town, B * A)
    rows, k = [], 0
    for b in range(B):
        scene = []
        for a in range(A):
            l = ll[k]
            if a % 2:
                l = town.succ[l][0]                                       # a junction lanelet, where lanelets overlap
            s = min(3.0 + 2.7 * k, town.length(l) - 3.0)
            scene.append(pose_row(town, l, s, left=0.2 * (a - 2)))
            k += 1
        rows.append(scene)
    return scene_states(rows)


def test_sampling_equals_the_model_on_the_ring(maps):
    from torchdrivesim_amd.goals import RouteGoal
    ring_map, ring = maps['ring']
    states, present = ring_batch(maps)
    length = torch.tensor([[200.0, 37.5, 200.0], [float('nan'), 200.0, 200.0]], device=DEV)
    goal = RouteGoal.sample(ring_map, states, present, seed=3, length=length)
    routes = model_routes(goal, [ring, ring], states, present.cpu().numpy())
    assert_routes(goal, routes)
    n = goal.n.cpu().numpy()
    assert n[0, 2] == 1 and routes[0][2].lanes == [4] and routes[0][2].length == 17.0, 'the fork\'s dead end'
    assert n[1].tolist() == [0, 0, 0], 'length nan, off the map, absent'
    assert goal.valid.cpu().tolist() == [[True, True, True], [False, False, False]] and not bool(goal.completed.any())
    assert routes[0][1].length == 37.5 and n[0, 1] >= 2
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        RouteGoal.sample(ring_map, states.cpu(), seed=3)


def test_sampling_equals_the_model_on_town01(maps):
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    states = town_batch(maps)
    ids = torch.tensor([7, 2 ** 40 + 1, 3], dtype=torch.int64, device=DEV)
    goal = RouteGoal.sample([town_map] * 3, states, seed=2 ** 63 + 11, scene_ids=ids)
    routes = model_routes(goal, [town] * 3, states)
    assert_routes(goal, routes)
    assert all(abs(r.length - 200.0) < 1e-9 and 1 <= r.n <= 10 for scene in routes for r in scene), 'Town01 has no dead end within 200 m'
    assert sum(r.n >= 4 for scene in routes for r in scene) >= 6
    assert len({tuple(r.lanes) for scene in routes for r in scene}) >= 12
    # points: the device's against the model's, float32 of the same float64
    arcs = torch.tensor([-1.0, 0.0, 0.1, 57.3, 123.456, 199.9, 200.0, 250.0], dtype=torch.float64, device=DEV)
    got = goal.points(arcs).cpu().numpy()
    for b in range(3):
        for a in range(5):
            assert bits(got[b, a]) == bits(rm.points(town, routes[b][a], arcs.cpu().numpy())), (b, a)


# ---------------------------------------------------------------------------------------------------------------- row independence
def route_snapshot(goal, b=slice(None)):
    return {k: v[b].clone() for k, v in goal._t.items() if k not in ('scene_ids', 'snap_xy', 'sc', 'snap_lane', 'snap_arc', 'snap_lateral')}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def make_sim(lanelet_maps, states, present=None, route_goals=None, waypoint_goals=None):
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    B, A = states.shape[:2]
    km = KinematicBicycle(dt=0.1)
    km.set_params(lr=torch.full((B, A), 1.4, device=DEV))
    km.set_state(states.clone())
    size = torch.tensor([4.5, 2.0], device=DEV).expand(B, A, 2).contiguous()
    present = torch.ones((B, A), dtype=torch.bool, device=DEV) if present is None else present
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    return Simulator(BirdviewMesh.empty(batch_size=B).to(DEV), km, size, present, cfg, renderer=renderer, lanelet_map=list(lanelet_maps),
                     route_goals=route_goals, waypoint_goals=waypoint_goals)


def test_rows_do_not_depend_on_their_batch(maps):
    from torchdrivesim_amd.goals import RouteGoal
    from torchdrivesim_amd.parallel import shard_simulator
    town_map, town = maps['town']
    ring_map, ring = maps['ring']
    lanelet_maps = [town_map, ring_map, town_map]
    states = town_batch(maps)
    states[1] = scene_states([pose_row(ring, 0, 2.5), pose_row(ring, 2, 7.0), pose_row(ring, 4, 3.0), pose_row(ring, 3, 12.5), pose_row(ring, 1, 9.0)])
    ids = torch.tensor([5, 9, 6], dtype=torch.int64, device=DEV)
    whole = RouteGoal.sample(lanelet_maps, states, seed=17, scene_ids=ids)
    assert whole.valid.all()
    # sub-batches sampled on their own
    for rows in ([1], [2, 0]):
        part = RouteGoal.sample([lanelet_maps[i] for i in rows], states[rows], seed=17, scene_ids=ids[rows])
        assert same(route_snapshot(part), route_snapshot(whole, rows)), rows
    # the whole batch steps once; selections, an extension and two shards of a copy made BEFORE that step give its rows
    sim = make_sim(lanelet_maps, states, route_goals=whole)
    picked = sim.select_batch_elements([2, 0], in_place=False)
    doubled = sim.extend(2, in_place=False)
    shards = [shard_simulator(sim, r, 2) for r in range(2)]
    action = torch.tensor([0.5, 0.05], device=DEV).expand(3, 5, 2).contiguous()
    sim.step(action)
    want = route_snapshot(sim.route_goals)
    assert bool((want['progress'] > 0).all()) and sim.compute_route_progress() is not None
    picked.step(action[[2, 0]])
    assert same(route_snapshot(picked.route_goals), {k: v[[2, 0]] for k, v in want.items()})
    doubled.step(action.repeat_interleave(2, 0))
    assert same(route_snapshot(doubled.route_goals), {k: v.repeat_interleave(2, 0) for k, v in want.items()})
    at = 0
    for shard in shards:
        n = shard.batch_size
        shard.step(action[at:at + n])
        assert same(route_snapshot(shard.route_goals), {k: v[at:at + n] for k, v in want.items()})
        at += n
    assert at == 3 and [s.batch_size for s in shards] == [2, 1]


def test_a_masked_resample_changes_only_the_masked_rows(maps):
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    states = town_batch(maps)
    goal = RouteGoal.sample(town_map, states, seed=23)
    step_and_compare(goal, [town] * 3, model_routes(goal, [town] * 3, states), states)      # stored progress and cursors are no longer all zero
    before = route_snapshot(goal)
    moved = states.roll(1, 1).contiguous()                                   # every agent stands where its neighbour stood
    mask = torch.zeros((3, 5), dtype=torch.bool, device=DEV)
    mask[0, 1] = mask[2, 4] = mask[1, 0] = True
    ids = torch.tensor([40, 41, 42], dtype=torch.int64, device=DEV)
    goal.resample(moved, scene_ids=ids, mask=mask)
    after = route_snapshot(goal)
    route_keys = ('lanes', 'n', 'start_arc', 'end_arc', 'offsets', 'length', 'cursor', 'stored', 'completed')
    for k in route_keys:
        assert torch.equal(after[k][~mask], before[k][~mask]), k
    assert not torch.equal(after['lanes'][mask], before['lanes'][mask])
    rows = mask.cpu().numpy()
    routes = model_routes(goal, [town] * 3, moved, rows=rows)
    assert_routes(goal, routes, 'resampled')
    assert [r is not None for scene in routes for r in scene].count(True) == 3


# ---------------------------------------------------------------------------------------------------------------- driving
def drive_pose(model, route, q, t, row, wide=False):
    """a pose near route arc q: beside the route by up to 0.6 m (6 m where `wide`), heading off it by up to 0.3 rad"""
    x, y = rm.point(model, route, q)
    ax, ay = rm.point(model, route, q + 0.5)
    if (ax, ay) == (x, y):
        x0, y0 = rm.point(model, route, q - 0.5)
        psi = math.atan2(y - y0, x - x0)
    else:
        psi = math.atan2(ay - y, ax - x)
    amp = 6.0 if wide else 0.6
    return [x + amp * math.sin(0.7 * t + row), y + amp * math.cos(0.4 * t + 2 * row), psi + 0.3 * math.sin(0.9 * t + row), 5.0]


def test_a_sixty_step_drive_equals_the_model(maps):
    """B = 2 x A = 4: scene 0 on the ring (two rows lap it two and a half times, one ends in the fork's dead end, one has no route), scene 1 on
    Town01 (one row absent from step 30 on).  Poses are the model's route points plus offsets; rows move at 3.7, 2.9, 1.3 and 4.0 m a step, so the
    fast ones arrive and stand past the end; row 1 of each scene strays 6 m off its route for steps 20 .. 25."""
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    ring_map, ring = maps['ring']
    models = [ring, town]
    seed = ring_seed(ring, [(4, 0, 0, 2.5), (4, 1, 3, 12.5)])
    states = scene_states([[pose_row(ring, 0, 2.5), pose_row(ring, 3, 12.5), pose_row(ring, 4, 3.0), [500.0, 500.0, 0.0, 0.0]]] * 2)
    states[1] = town_batch(maps)[2, :4]                                    # starts in and before junctions: routes of four lanelets and more
    ids = torch.tensor([4, 11], dtype=torch.int64, device=DEV)
    goal = RouteGoal.sample([ring_map, town_map], states, seed=seed, scene_ids=ids, lookahead=16, spacing=4.0)
    routes = model_routes(goal, models, states)
    assert_routes(goal, routes)
    assert routes[0][0].n == 11 and routes[0][1].n == 11 and routes[0][2].lanes == [4] and routes[0][3].n == 0
    assert all(r.n >= 3 and abs(r.length - 200.0) < 1e-9 for r in routes[1])
    rate = (3.7, 2.9, 1.3, 4.0)
    present = torch.ones((2, 4), dtype=torch.bool, device=DEV)
    seen_off = seen_reached = 0
    cursors = []
    for t in range(60):
        rows = [[drive_pose(models[b], routes[b][a], t * rate[a], t, a, wide=(a == 1 and 20 <= t <= 25)) if routes[b][a].n else [500.0, 500.0, 0.1 * t, 0.0]
                 for a in range(4)] for b in range(2)]
        if t == 30:
            present[1, 2] = False
        got = step_and_compare(goal, models, routes, scene_states(rows), present, what=f'step {t}')
        seen_off += int(got['off_route'].sum())
        seen_reached += int(got['reached'].sum())
        cursors.append(goal.cursor.cpu().numpy().copy())
        if t == 0:
            assert np.abs(got['advance']).max() < 1.0, 'the first advance is measured from the route\'s start, where the agent stands'
    cursors = np.stack(cursors)
    assert (np.diff(cursors, axis=0) >= 0).all(), 'a cursor never decreases'
    assert cursors[-1, 0, 0] == 10 and cursors[-1, 0, 1] >= 8, 'two laps and more: pieces 0 .. 10 of the ring'
    assert seen_off >= 2 and seen_reached >= 10
    done = goal.completed.cpu().numpy()
    assert done[0, 0] and done[1, 0] and done[1, 3] and not done[0, 3] and not done[1, 2]


def test_windows_wider_than_a_wave_and_of_one_segment(maps):
    """rows whose window holds more segments than a wavefront has lanes (Town01's long lanelets, walked end to end), a route of a single segment,
    and a route that ends inside its first lanelet"""
    from torchdrivesim_amd.goals import RouteGoal
    town_map, town = maps['town']
    ring_map, ring = maps['ring']
    wide = None
    for l in sorted(range(len(town)), key=lambda l: -len(town.cl[l])):
        if not town.eligible(l) or town.flag[l]:
            continue
        r = rm.sample(town, l, 1.0, 200.0, 29, 0, 0)
        if r.n >= 3 and sum(len(town.cl[x]) - 1 for x in r.lanes[:3]) > 64:
            wide = l
            break
    assert wide is not None, 'Town01 has routes with more than 64 segments in a window'
    states = scene_states([[pose_row(town, wide, 1.0), pose_row(town, long_lanelets(town, 1)[0], 5.0)],
                           [pose_row(ring, 2, 6.0), pose_row(ring, 1, 3.0)]])
    length = torch.tensor([[200.0, 30.0], [3.0, 12.0]], device=DEV)
    goal = RouteGoal.sample([town_map, ring_map], states, seed=29, length=length, lookahead=32, spacing=1.5)
    models = [town, ring]
    routes = model_routes(goal, models, states)
    assert_routes(goal, routes)
    assert sum(len(town.cl[x]) - 1 for x in routes[0][0].lanes[:3]) > 64
    assert routes[1][0].lanes == [2] and (routes[1][0].start_arc, routes[1][0].end_arc) == (6.0, 9.0), 'inside one segment of 5 m'
    assert routes[0][1].n == 1 and routes[1][1].lanes == [1], 'routes that end inside their first lanelet'
    for t in range(12):
        rows = [[drive_pose(models[b], routes[b][a], t * (17.0, 2.5)[a] * (1.0 if b == 0 else 0.1), t, a) for a in range(2)] for b in range(2)]
        step_and_compare(goal, models, routes, scene_states(rows), what=f'step {t}')
    assert goal.cursor.cpu()[0, 0] >= 2


def test_bad_arguments_are_refused(maps):
    from torchdrivesim_amd import _native
    from torchdrivesim_amd.goals import RouteGoal
    ring_map, _ = maps['ring']
    states, _ = ring_batch(maps)
    for kw in (dict(lookahead=33), dict(lookahead=-1), dict(spacing=float('nan')), dict(goal_tolerance=-1.0), dict(off_route_distance=float('inf'))):
        with pytest.raises(_native.TdsError) as e:
            RouteGoal.sample(ring_map, states, seed=1, **kw)
        assert e.value.code == _native.E_INVAL
    goal = RouteGoal.sample(ring_map, states, seed=1, lookahead=0)
    out = goal.step(states)
    assert out.lookahead.shape == (2, 3, 0, 2) and bool((out.progress[0] >= 0).all())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        goal.step(states.cpu())


# ---------------------------------------------------------------------------------------------------------------- the simulator
def test_a_captured_step_with_route_goals_replays_the_eager_steps(maps):
    """Simulator.step with route_goals in a HIP graph: the route step allocates nothing and synchronises nothing, so three replays give what three
    eager steps give"""
    from torchdrivesim_amd.goals import RouteGoal
    town_map, _ = maps['town']
    ring_map, _ = maps['ring']
    lanelet_maps = [town_map, ring_map]
    base = town_batch(maps, B=2, A=3)
    _, ring = maps['ring']
    base[1] = scene_states([pose_row(ring, 0, 2.5), pose_row(ring, 2, 7.0), pose_row(ring, 3, 12.5)])
    sims = []
    for _ in range(2):
        goal = RouteGoal.sample(lanelet_maps, base, seed=31, length=60.0)
        sims.append(make_sim(lanelet_maps, base, route_goals=goal))
    sim, ref = sims
    state = base.clone()
    action = torch.tensor([1.0, 0.1], device=DEV).expand(2, 3, 2).contiguous()

    def step(s, st):
        s.kinematic_model.set_state(st)
        s.step(action)
        return s.get_state()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(sim, state)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        step(ref, state.clone())
    torch.cuda.synchronize()
    assert same(route_snapshot(sim.route_goals), route_snapshot(ref.route_goals))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        state_next = step(sim, state).clone()
    for i in range(3):
        new = step(ref, state.clone())
        want = route_snapshot(ref.route_goals)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(state_next, new), i
        assert same(route_snapshot(sim.route_goals), want), i
        assert bool((want['advance'] > 0).all()) if i else True
        state.copy_(state_next)
    progress = ref.compute_route_progress()
    assert progress is ref.route_goals.last_progress or torch.equal(progress.progress, ref.route_goals.last_progress.progress)
    assert bool((progress.progress > 0.2).all())


def test_routes_are_drawn_as_goal_discs(maps):
    """waypoint_goal(4.0) through the renderer at 64 x 64 equals a hand-made WaypointGoal holding the model's points"""
    from torchdrivesim_amd.goals import RouteGoal, WaypointGoal
    from torchdrivesim_amd.utils import Resolution
    ring_map, ring = maps['ring']
    states = scene_states([[pose_row(ring, 0, 2.5), pose_row(ring, 4, 3.0)]])
    seed = ring_seed(ring, [(0, 0, 0, 2.5)])
    length = torch.tensor([[50.0, 200.0]], device=DEV)
    goal = RouteGoal.sample(ring_map, states, seed=seed, length=length)
    routes = model_routes(goal, [ring], states)
    assert routes[0][0].length == 50.0 and routes[0][1].length == 17.0
    drawn = goal.waypoint_goal(4.0)
    N = int(50.0 / 4.0) + 1
    assert drawn.waypoints.shape == (1, 2, N, 1, 2) and drawn.mask.shape == (1, 2, N, 1)
    arcs = np.arange(N) * 4.0
    pts = np.stack([rm.points(ring, routes[0][a], arcs) for a in range(2)])[None, :, :, None, :]
    mask = np.stack([arcs <= routes[0][a].length for a in range(2)])[None, :, :, None]
    assert mask.sum() == 13 + 5
    by_hand = WaypointGoal(torch.tensor(pts, device=DEV), torch.tensor(mask, device=DEV))
    assert torch.equal(drawn.waypoints, by_hand.waypoints) and torch.equal(drawn.mask, by_hand.mask)
    images = []
    for goals in (drawn, by_hand, None):
        sim = make_sim([ring_map], states, waypoint_goals=goals)
        images.append(sim.render_egocentric(res=Resolution(64, 64), fov=35.0, n_subsequent_waypoints=N).clone())
    assert torch.equal(images[0], images[1])
    assert not torch.equal(images[0], images[2]), 'the discs are there'
