"""Routes to a destination on the device (csrc/route_to.hip `tds_lane_distances_f64`, `tds_route_to_multi`; goals.RouteGoal.to / resample_to)
against the float64 model of their definition (tests/route_to_model.py).  The model is fed the (lane, arc) the device's snap found for the very
poses the kernels read (the snap has its own tests, tests/test_gpu_lane_follow.py).

The bar: distance tables, lanes, n, cursor and the flags equal; arcs, offsets, lengths, `rest` and every float output equal BIT FOR BIT (the
kernels are float64 + and compares built with -ffp-contract=off, the model the same expressions in the same order).  No row is excepted."""
import math
import os

import numpy as np
import pytest
import torch

import route_model as rm
import route_to_model as rt
import test_gpu_route_goals as base
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = base.DEV
INF = math.inf
bits, scene_states, pose_row = base.bits, base.scene_states, base.pose_row


@pytest.fixture(scope='module')
def maps():
    """name -> (LaneletMap, model, the model's distance table)"""
    from torchdrivesim_amd import lanelet2
    out = {k: lanelet2.load_lanelet_map(os.path.join(GOLDEN, f), origin=(0.0, 0.0))
           for k, f in (('Town01', 'carla_Town01.osm.gz'), ('Town02', 'carla_Town02.osm.gz'), ('testing', 'testing_lanelet2map.osm'))}
    out['ring'], out['diamond'] = rm.ring_with_fork(), rt.diamond()
    models = {k: rm.Lanes(m) for k, m in out.items()}
    return {k: (m, models[k], rt.distance_table(models[k])) for k, m in out.items()}


def device_table(lanelet_map):
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import LANELET_TAGS_TO_EXCLUDE
    return _ops.lane_distances(lanelet_map.table(torch.device(DEV), LANELET_TAGS_TO_EXCLUDE))


def model_deals(goal, scenes, present=None, rows=None):
    """the model's (route, rest) of every row, from the snap the device made of the agents' poses and the destinations the goal object stores;
    scenes: per scene (map, model, table) or None"""
    t = {k: goal._t[k].cpu().numpy() for k in ('snap_lane', 'snap_arc', 'dest_lane', 'dest_arc')}
    B, A = t['snap_lane'].shape
    out = [[None] * A for _ in range(B)]
    for b in range(B):
        for a in range(A):
            if rows is not None and not rows[b][a]:
                continue
            _, model, table = scenes[b] if scenes[b] is not None else (None, None, None)
            out[b][a] = rt.deal(model, table, t['snap_lane'][b, a], t['snap_arc'][b, a], t['dest_lane'][b, a], t['dest_arc'][b, a],
                                True if present is None else bool(present[b][a]))
    return out


def assert_deals(tensors, deals, what=''):
    """route tensors, state and `rest` (a RouteGoal or a dict of tensors) against the model's deals"""
    routes = [[None if d is None else d[0] for d in scene] for scene in deals]
    holder = tensors if hasattr(tensors, '_t') else type('T', (), {'_t': tensors})()
    base.assert_routes(holder, routes, what)
    rest = holder._t['rest'].cpu().numpy()
    for b, scene in enumerate(deals):
        for a, d in enumerate(scene):
            if d is not None:
                assert bits(rest[b, a]) == bits(np.float64(d[1])), (what, b, a, rest[b, a], d[1])
    return routes


# ---------------------------------------------------------------------------------------------------------------- distance tables
@pytest.mark.parametrize('name', ['ring', 'diamond', 'testing', 'Town01', 'Town02'])
def test_distance_tables_equal_the_model(maps, name):
    lanelet_map, model, table = maps[name]
    got = device_table(lanelet_map)
    assert got.shape == (len(model), len(model)) and got.dtype == torch.float64
    assert bits(got.cpu().numpy()) == bits(table)
    assert device_table(lanelet_map) is got, 'built once per table'


def test_graphs_the_distance_kernel_cannot_hold_are_refused():
    """a chain of TDS_ROUTE_MAX_GRAPH + 1 lanelets is TDS_ELIMIT, from the binding's own check and from the entry point (which launches
    nothing); a table without a successor graph is TDS_EINVAL"""
    from torchdrivesim_amd import _native as nat, _ops
    from torchdrivesim_amd.lanelet2 import LaneTable
    L = nat.ROUTE_MAX_GRAPH + 1
    x = np.arange(L, dtype=np.float64)[:, None] * 2.0
    poly = np.stack([np.concatenate([x, np.full((L, 1), 1.0)], 1), np.concatenate([x + 2.0, np.full((L, 1), 1.0)], 1),
                     np.concatenate([x + 2.0, np.full((L, 1), -1.0)], 1), np.concatenate([x, np.full((L, 1), -1.0)], 1)], 1).reshape(-1, 2)
    cl = np.stack([np.concatenate([x, np.zeros((L, 2))], 1), np.concatenate([x + 2.0, np.zeros((L, 2))], 1)], 1).reshape(-1, 3)
    succ_start = np.minimum(np.arange(L + 1), L - 1).astype(np.int32)
    chain = LaneTable(poly, np.arange(L + 1, dtype=np.int32) * 4, cl, np.arange(L + 1, dtype=np.int32) * 2, np.zeros(L, np.int32), succ_start,
                      np.arange(1, L, dtype=np.int32))
    handle = _ops.LaneTableHandle(chain, DEV)
    with pytest.raises(nat.TdsError) as e:
        _ops.lane_distances(handle)
    assert e.value.code == nat.E_LIMIT
    with pytest.raises(nat.TdsError) as e:
        nat.call('tds_lane_distances_f64', handle.device, handle.handle, torch.zeros(1, dtype=torch.float64, device=DEV))
    assert e.value.code == nat.E_LIMIT and '2049 lanelets' in str(e.value)
    bare = _ops.LaneTableHandle(LaneTable(poly[:8], np.array([0, 4, 8], np.int32), cl[:4], np.array([0, 2, 4], np.int32), np.zeros(2, np.int32)), DEV)
    with pytest.raises(nat.TdsError) as e:
        _ops.lane_distances(bare)
    assert e.value.code == nat.E_INVAL and 'successor' in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- the cases of the definition
def test_every_case_of_the_definition_on_the_ring_and_the_diamond(maps):
    """B = 3 (ring, diamond, ring) x A = 5 through the entry point itself, lanes and arcs given: ahead and behind on one lanelet, adjacent lanelets
    with b = 0 and b = len, a start in the dead end (its destination cannot be reached), the tie, a way round, an absent row, a masked row, lane
    indices out of range on either side, arcs that are clamped, a route of zero length"""
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.goals import RouteGoal
    from torchdrivesim_amd.lanelet2 import lane_set_for
    scenes = [maps['ring'], maps['diamond'], maps['ring']]
    rows = [[(1, 5.0, 1, 12.5), (1, 12.5, 1, 5.0), (1, 5.0, 2, 0.0), (1, 5.0, 2, 20.0), (4, 3.0, 0, 1.0)],
            [(0, 2.0, 3, 4.0), (2, 1.0, 1, 1.0), (3, 1.0, 0, 0.0), (0, 1.0, 1, 1.0), (0, 1.0, 1, 1.0)],
            [(3, 2.0, 4, 7.0), (7, 0.0, 1, 1.0), (1, 0.0, -1, 1.0), (0, 99.0, 2, math.nan), (1, 5.0, 1, 5.0)]]
    col = lambda i, dtype: torch.tensor([[r[i] for r in scene] for scene in rows], dtype=dtype, device=DEV)
    lane, arc, dest_lane, dest_arc = col(0, torch.int32), col(1, torch.float64), col(2, torch.int32), col(3, torch.float64)
    present = torch.ones((3, 5), dtype=torch.bool, device=DEV)
    mask = torch.ones((3, 5), dtype=torch.bool, device=DEV)
    present[1, 3], mask[1, 4] = False, False
    route = RouteGoal._buffers(3, 5, 0, torch.device(DEV))
    route['rest'] = torch.zeros((3, 5), dtype=torch.float64, device=DEV)
    for k in ('lanes', 'n', 'cursor'):
        route[k].fill_(7)
    for k in ('start_arc', 'end_arc', 'offsets', 'length', 'stored', 'rest'):
        route[k].fill_(-3.25)
    route['completed'].fill_(1)
    lane_set = lane_set_for([s[0] for s in scenes], 3, torch.device(DEV))
    _ops.route_to(lane_set, lane, arc, dest_lane, dest_arc, present, mask, route)
    deals = [[rt.deal(scenes[b][1], scenes[b][2], *rows[b][a], present=bool(present[b, a])) if bool(mask[b, a]) else None for a in range(5)]
             for b in range(3)]
    assert_deals(route, deals)
    got = {k: v.cpu().numpy() for k, v in route.items()}
    assert got['n'].tolist() == [[1, 5, 1, 2, 0], [3, 4, 1, 0, 7], [3, 0, 0, 2, 0]]
    assert got['lanes'][1, 0, :3].tolist() == [0, 1, 3], 'the tie takes the first successor'
    assert got['lanes'][1, 1, :4].tolist() == [2, 3, 0, 1] and got['lanes'][0, 1, :5].tolist() == [1, 2, 3, 0, 1]
    assert got['rest'][0].tolist() == [0.0, 0.0, 0.0, 0.0, INF] and got['rest'][2].tolist() == [0.0, INF, INF, 0.0, 0.0]
    assert got['rest'][1, 3] == INF and got['length'][2, 3] == 20.0, 'absent; start clamped to the end of lanelet 0, destination arc NaN to 0'
    for k in ('start_arc', 'end_arc', 'length', 'stored', 'rest'):                     # the masked row keeps everything
        assert got[k][1, 4] == -3.25, k
    assert got['cursor'][1, 4] == 7 and got['completed'][1, 4] == 1 and (got['lanes'][1, 4] == 7).all() and (got['offsets'][1, 4] == -3.25).all()


# ---------------------------------------------------------------------------------------------------------------- the towns
def town_pairs(scenes, A, seed):
    """per scene A random usable (lane, arc) starts and destinations -> (states (B, A, 4), destination lanes, destination arcs)"""
    g = np.random.default_rng(seed)
    states, lanes, arcs = [], [], []
    for _, model, _ in scenes:
        ok = [l for l in range(len(model)) if rt.usable(model, l)]
        start, dest = g.choice(ok, A), g.choice(ok, A)
        u, w = g.uniform(0.05, 0.95, A), g.uniform(0.0, 1.0, A)
        states.append([pose_row(model, int(l), float(x) * model.length(int(l))) for l, x in zip(start, u)])
        lanes.append([int(l) for l in dest])
        arcs.append([float(x) * model.length(int(l)) for l, x in zip(dest, w)])
    return scene_states(states), torch.tensor(lanes, dtype=torch.int32, device=DEV), torch.tensor(arcs, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize('towns', [('Town01',), ('Town01', 'Town02')])
def test_routes_on_the_towns_equal_the_model(maps, towns):
    """B = 8 x A = 32 on Town01, then with the scenes alternating Town01 / Town02 (124 and 88 lanelets: a wrong table pointer or row stride
    shows).  numpy seed 2024 was chosen on the CPU, with the model alone, to give at least 8 truncated and 8 complete rows in either batch."""
    from torchdrivesim_amd.goals import RouteGoal
    scenes = [maps[towns[b % len(towns)]] for b in range(8)]
    states, dest_lanes, dest_arcs = town_pairs(scenes, 32, 2024)
    goal = RouteGoal.to([s[0] for s in scenes], states, destination_lanes=dest_lanes, destination_arcs=dest_arcs)
    assert torch.equal(goal.destination_lanes, dest_lanes) and torch.equal(goal.destination_arcs, dest_arcs)
    deals = model_deals(goal, scenes)
    routes = assert_deals(goal, deals)
    flat = [d for scene in deals for d in scene]
    cut, complete = sum(0.0 < d[1] < INF for d in flat), sum(d[1] == 0.0 and d[0].n > 0 for d in flat)
    assert cut >= 8 and complete >= 8, (cut, complete)
    assert goal.truncated.sum().item() == cut and goal.valid.sum().item() == sum(d[0].n > 0 for d in flat)
    assert bool((goal.rest == goal._t['rest']).all()) and max(d[0].n for d in flat) == 16
    # the end point of every route: the device's against the model's, float32 of the same float64; a complete route ends at its destination
    ends = goal.points(goal.length.unsqueeze(-1)).cpu().numpy()
    for b, scene in enumerate(routes):
        for a, r in enumerate(scene):
            assert bits(ends[b, a]) == bits(rm.points(scenes[b][1], r, [r.length])), (b, a)
            if deals[b][a][1] == 0.0 and r.n > 0:
                x, y = scenes[b][1].pose(int(dest_lanes[b, a]), float(dest_arcs[b, a]))[:2]
                assert abs(ends[b, a, 0, 0] - x) < 1e-3 and abs(ends[b, a, 0, 1] - y) < 1e-3, (b, a)


def test_destination_poses_equal_their_snap(maps):
    """RouteGoal.to(destination=poses) holds what the lane / arc form holds when it is fed snap_to_lanes(poses); a pose off the map is no destination"""
    from torchdrivesim_amd.goals import RouteGoal
    from torchdrivesim_amd.lanelet2 import snap_to_lanes
    scenes = [maps['Town01'], maps['Town02']]
    lanelet_maps = [s[0] for s in scenes]
    states, lanes, arcs = town_pairs(scenes, 8, 7)
    poses = scene_states([[pose_row(scenes[b][1], int(lanes[b, a]), float(arcs[b, a]), left=0.3) for a in range(8)] for b in range(2)])[..., :3].contiguous()
    poses[1, 5, :2] = 5000.0
    by_pose = RouteGoal.to(lanelet_maps, states, poses)
    lane, arc, _ = snap_to_lanes(lanelet_maps, poses)
    assert int(lane[1, 5]) == -1 and int((lane >= 0).sum()) == 15
    by_lane = RouteGoal.to(lanelet_maps, states, destination_lanes=lane, destination_arcs=arc)
    for k in ('lanes', 'n', 'start_arc', 'end_arc', 'offsets', 'length', 'rest', 'dest_lane', 'dest_arc', 'cursor', 'stored', 'completed'):
        assert torch.equal(by_pose._t[k], by_lane._t[k]), k
    assert not bool(by_pose.valid[1, 5]) and by_pose.rest[1, 5].item() == INF and int(by_pose.valid.sum()) >= 14
    assert_deals(by_pose, model_deals(by_pose, scenes))
    for bad in (dict(), dict(destination=poses, destination_lanes=lane, destination_arcs=arc), dict(destination_lanes=lane)):
        with pytest.raises(ValueError):
            RouteGoal.to(lanelet_maps, states, **bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        RouteGoal.to(lanelet_maps, states.cpu(), poses)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        RouteGoal.to(lanelet_maps, states, poses.cpu())
    sampled = RouteGoal.sample(lanelet_maps, states, seed=1)
    assert 'dest_lane' not in sampled._t and 'rest' not in sampled._t, 'sampled routes hold what they held'
    with pytest.raises(RuntimeError, match='no stored destinations'):
        sampled.resample_to(states)
    with pytest.raises(RuntimeError, match='resample_to'):
        by_pose.resample(states)


# ---------------------------------------------------------------------------------------------------------------- driving
def short_pairs(model, table, count, lo=60.0, hi=130.0):
    """(start lanelet, destination lanelet) pairs whose routes are between lo and hi metres long and hold at least three lanelets"""
    out = []
    for l0 in range(len(model)):
        for t in range(len(model)):
            r, rest = rt.deal(model, table, l0, 3.0, t, 2.0)
            if rest == 0.0 and r.n >= 3 and lo <= r.length <= hi:
                out.append((l0, t))
                break
        if len(out) == count:
            return out
    raise AssertionError('Town01 has such pairs')


def test_progress_along_a_dealt_route(maps):
    """the progress kernel on dealt routes: agents step along the model's route points 2 m at a time; every output equals the model of route goals
    bit for bit, progress never decreases and `reached` fires within goal_tolerance of the destination"""
    from torchdrivesim_amd.goals import RouteGoal
    lanelet_map, model, table = maps['Town01']
    pairs = short_pairs(model, table, 4)
    states = scene_states([[pose_row(model, l0, 3.0) for l0, _ in pairs]])
    dest_lanes = torch.tensor([[t for _, t in pairs]], dtype=torch.int32, device=DEV)
    dest_arcs = torch.full((1, 4), 2.0, dtype=torch.float64, device=DEV)
    goal = RouteGoal.to(lanelet_map, states, destination_lanes=dest_lanes, destination_arcs=dest_arcs, goal_tolerance=2.0, lookahead=8)
    routes = assert_deals(goal, model_deals(goal, [maps['Town01']]))
    assert all(r.n >= 3 for r in routes[0]) and not bool(goal.truncated.any())
    steps = int(max(r.length for r in routes[0]) / 2.0) + 2
    last = np.zeros(4, np.float32)
    first_reached = [None] * 4
    for i in range(steps):
        rows = [[None] * 4]
        for a, r in enumerate(routes[0]):                                    # on the route exactly, heading along it
            x, y = rm.point(model, r, 2.0 * i)
            nx, ny = rm.point(model, r, 2.0 * i + 0.5)
            px, py = rm.point(model, r, 2.0 * i - 0.5)
            rows[0][a] = [x, y, math.atan2(ny - py, nx - px), 5.0]
        got = base.step_and_compare(goal, [model], routes, scene_states(rows), what=f'step {i}')
        assert (got['progress'][0] >= last).all(), i
        last = got['progress'][0].copy()
        for a, r in enumerate(routes[0]):
            if got['reached'][0, a] and first_reached[a] is None:
                first_reached[a] = i
                assert r.length - 2.0 * i <= 2.0 + 1e-3 and r.length - 2.0 * (i - 1) > 2.0 - 1e-3, (a, i, r.length)
    assert None not in first_reached and bool(goal.completed.all())
    x, y = model.pose(int(dest_lanes[0, 0]), 2.0)[:2]
    end = goal.points(goal.length.unsqueeze(-1)).cpu().numpy()[0, 0, 0]
    assert abs(end[0] - x) < 1e-3 and abs(end[1] - y) < 1e-3


# ---------------------------------------------------------------------------------------------------------------- re-planning
def test_a_masked_resample_to_changes_only_the_masked_rows(maps):
    from torchdrivesim_amd.goals import RouteGoal
    scenes = [maps['Town01'], maps['Town02']]
    lanelet_maps = [s[0] for s in scenes]
    states, lanes, arcs = town_pairs(scenes, 8, 3)
    goal = RouteGoal.to(lanelet_maps, states, destination_lanes=lanes, destination_arcs=arcs)
    goal.step(states)                                                        # stored progress is no longer all zero
    before = base.route_snapshot(goal)
    moved, new_lanes, new_arcs = town_pairs(scenes, 8, 4)
    mask = torch.zeros((2, 8), dtype=torch.bool, device=DEV)
    mask[0, 1] = mask[1, 6] = mask[1, 0] = True
    goal.resample_to(moved, mask=mask, destination_lanes=new_lanes, destination_arcs=new_arcs)
    after = base.route_snapshot(goal)
    keys = ('lanes', 'n', 'start_arc', 'end_arc', 'offsets', 'length', 'cursor', 'stored', 'completed', 'rest', 'dest_lane', 'dest_arc')
    for k in keys:
        assert torch.equal(after[k][~mask], before[k][~mask]), k
    assert torch.equal(after['dest_lane'][mask], new_lanes[mask]) and not torch.equal(after['lanes'][mask], before['lanes'][mask])
    rows = mask.cpu().numpy()
    deals = model_deals(goal, scenes, rows=rows)
    assert_deals(goal, deals, 'masked')
    assert sum(d is not None for scene in deals for d in scene) == 3
    goal.resample_to(moved)                                                  # all rows, to the destinations the object stores
    assert_deals(goal, model_deals(goal, scenes), 'all')
    assert torch.equal(goal.destination_lanes[mask], new_lanes[mask]) and torch.equal(goal.destination_lanes[~mask], lanes[~mask])


def test_truncated_routes_are_continued_from_their_end(maps):
    """agents that stand at the end of a truncated route have completed it; `resample_to(mask=completed & truncated)` deals them the rest, which
    reaches the destination"""
    from torchdrivesim_amd.goals import RouteGoal
    scenes = [maps['Town01']] * 2
    states, lanes, arcs = town_pairs(scenes, 32, 2024)
    goal = RouteGoal.to(maps['Town01'][0], states, destination_lanes=lanes, destination_arcs=arcs)
    cut = goal.truncated.clone()
    assert int(cut.sum()) >= 4
    first = model_deals(goal, scenes)
    model = maps['Town01'][1]
    at_end = states.clone()
    for b in range(2):
        for a in range(32):
            r = first[b][a][0]
            if r.n:                                                           # half a metre before the end of the route, heading along it
                at_end[b, a] = torch.tensor(pose_row(model, r.lanes[-1], max(r.end_arc - 0.5, 0.0)), device=DEV)
    goal._t['cursor'].copy_((goal.n - 1).clamp(min=0))                        # as if driven there: the window of a step is the cursor's piece and two more
    out = goal.step(at_end)
    assert bool(out.reached[goal.valid].all()) and bool((goal.completed == goal.valid).all())
    mask = goal.completed & goal.truncated
    assert torch.equal(mask, cut)
    before = base.route_snapshot(goal)
    goal.resample_to(at_end, mask=mask)
    second = model_deals(goal, scenes, rows=mask.cpu().numpy())
    assert_deals(goal, second, 'continued')
    after = base.route_snapshot(goal)
    for k in ('lanes', 'length', 'rest', 'completed', 'stored', 'cursor'):
        assert torch.equal(after[k][~mask], before[k][~mask]), k
    assert not bool(goal.completed[mask].any())
    snapped = goal._t['snap_lane'].cpu().numpy()
    arrived = 0
    for b in range(2):
        for a in range(32):
            # where the snap finds the lanelet the first route ended on (in a junction the heading may prefer one that overlaps it), the second
            # route is what was left of the first: it reaches the destination, and is `rest` long plus the half metre still to go
            if second[b][a] is not None and snapped[b, a] == first[b][a][0].lanes[-1]:
                r, rest = second[b][a]
                assert rest == 0.0 and r.n >= 1 and (r.lanes[-1] == int(lanes[b, a]) or float(arcs[b, a]) == 0.0)
                assert abs((r.length - 0.5) - first[b][a][1]) < 1e-3, (b, a, r.length, first[b][a][1])
                arrived += 1
    assert arrived >= 4


# ---------------------------------------------------------------------------------------------------------------- rows, shards, capture
def mixed_batch(maps):
    """B = 3 (Town01, ring, Town01) x A = 4 -> (lanelet maps, scenes, states, destination lanes, arcs)"""
    scenes = [maps['Town01'], maps['ring'], maps['Town01']]
    states, lanes, arcs = town_pairs(scenes, 4, 12)
    return [s[0] for s in scenes], scenes, states, lanes, arcs


def test_rows_do_not_depend_on_their_batch(maps):
    from torchdrivesim_amd.goals import RouteGoal
    from torchdrivesim_amd.parallel import shard_simulator
    lanelet_maps, scenes, states, lanes, arcs = mixed_batch(maps)
    whole = RouteGoal.to(lanelet_maps, states, destination_lanes=lanes, destination_arcs=arcs)
    assert_deals(whole, model_deals(whole, scenes))
    assert int(whole.valid.sum()) >= 9
    for rows in ([1], [2, 0]):                                               # sub-batches dealt on their own
        part = RouteGoal.to([lanelet_maps[i] for i in rows], states[rows], destination_lanes=lanes[rows], destination_arcs=arcs[rows])
        assert base.same(base.route_snapshot(part), base.route_snapshot(whole, rows)), rows
    # selections and two shards of a copy carry the destinations: dealt again from new poses and stepped, they give the whole batch's rows
    sim = base.make_sim(lanelet_maps, states, route_goals=whole)
    picked = sim.select_batch_elements([2, 0], in_place=False)
    shards = [shard_simulator(sim, r, 2) for r in range(2)]
    moved = states.roll(1, 1).contiguous()
    action = torch.tensor([0.5, 0.05], device=DEV).expand(3, 4, 2).contiguous()

    def replan_and_step(s, rows):
        s.kinematic_model.set_state(moved[rows].clone())
        s.route_goals.resample_to(moved[rows])
        s.step(action[rows])
        return base.route_snapshot(s.route_goals)

    want = replan_and_step(sim, slice(None))
    assert base.same(replan_and_step(picked, [2, 0]), {k: v[[2, 0]] for k, v in want.items()})
    at = 0
    for shard in shards:
        n = shard.batch_size
        assert base.same(replan_and_step(shard, slice(at, at + n)), {k: v[at:at + n] for k, v in want.items()})
        at += n
    assert at == 3 and bool((want['progress'][want['n'] > 0] >= 0).all())


def test_a_captured_replan_and_step_replays_the_eager_ones(maps):
    """resample_to + Simulator.step in a HIP graph (one stream, no parallel branches): with the distance tables built beforehand they allocate
    nothing and synchronise nothing, so three replays give what three eager rounds give"""
    from torchdrivesim_amd.goals import RouteGoal
    lanelet_maps, scenes, base_states, lanes, arcs = mixed_batch(maps)
    sims = []
    for _ in range(2):
        goal = RouteGoal.to(lanelet_maps, base_states, destination_lanes=lanes, destination_arcs=arcs)
        sims.append(base.make_sim(lanelet_maps, base_states, route_goals=goal))
    sim, ref = sims
    state = base_states.clone()
    action = torch.tensor([1.0, 0.1], device=DEV).expand(3, 4, 2).contiguous()
    mask = torch.zeros((3, 4), dtype=torch.bool, device=DEV)
    mask[:, ::2] = True

    def round_of(s, st):
        s.kinematic_model.set_state(st)
        s.route_goals.resample_to(st, mask=mask)
        s.step(action)
        return s.get_state()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            round_of(sim, state)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        round_of(ref, state.clone())
    torch.cuda.synchronize()
    assert base.same(base.route_snapshot(sim.route_goals), base.route_snapshot(ref.route_goals))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        state_next = round_of(sim, state).clone()
    for i in range(3):
        new = round_of(ref, state.clone())
        want = base.route_snapshot(ref.route_goals)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(state_next, new), i
        assert base.same(base.route_snapshot(sim.route_goals), want), i
        state.copy_(state_next)
    assert int(want['n'][mask].sum()) > 0 and bool((want['progress'][mask] < 3.0).all()), 'the masked rows start again every round'
