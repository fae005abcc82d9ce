"""Lane-following NPC traffic on the device (csrc/lanes.hip `tds_lane_snap`, csrc/follow.hip `tds_lane_follow_step`, behavior/lane_follow.py) against
the float64 model of its definition (tests/lane_follow_model.py), which is fed the very entities -- [sin, cos] included -- the controller hands
to the kernel.

The bar: `lane`, `hops`, `leader` equal; `arc`, `speed`, `x`, `y`, `[sin, cos]` equal BIT FOR BIT (the kernel is float64 + - * / sqrt built with
-ffp-contract=off, the model the same expressions in the same order); `psi`, a float64 atan2 rounded once, within one float32 ulp.  No row is
excepted."""
import math
import os

import numpy as np
import pytest
import torch

import lane_follow_model as lf
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32


@pytest.fixture(scope='module')
def towns():
    from torchdrivesim_amd import lanelet2
    maps = [lanelet2.load_lanelet_map(os.path.join(GOLDEN, f'carla_Town0{k}.osm.gz'), origin=(0.0, 0.0)) for k in (1, 2)]
    return maps, [lf.Lanes(m) for m in maps]


def long_lanelets(model, n=8):
    """the n longest lanelets one can drive on, longest first"""
    ok = [l for l in range(len(model)) if model.eligible(l) and not model.flag[l]]
    return sorted(ok, key=lambda l: -model.length(l))[:n]


def pose_row(model, lanelet, arc, speed, left=0.0, reverse=False):
    """[x, y, psi, speed] on a centre line, optionally moved `left` metres off it and turned round"""
    x, y, psi, sn, cs = (float(v) for v in model.pose(lanelet, arc))
    x, y = x - left * sn, y + left * cs
    return [x, y, psi + (math.pi if reverse else 0.0), speed]


def make_sim(towns, which, A, N, seed, edit=None, dt=0.1, lights=None, agents=None, **ctrl_kw):
    """len(which) scenes, scene b on town which[b]; A exposed agents and N lane-following NPCs placed by heuristic_initialize_batch, then
    edit(states (B, A + N, 4), present (B, A + N)) may move them by hand; agents: (B, A', 4) states that REPLACE the exposed agents"""
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    from torchdrivesim_amd.behavior.lane_follow import LaneFollowingNPCController
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    maps, _ = towns
    B = len(which)
    lanes = [maps[w] for w in which]
    attributes, states, placed = heuristic_initialize_batch(lanes, B, A + N, seed=seed, device=DEV)
    assert bool(placed.all())
    states, placed = states.clone(), placed.clone()
    if edit is not None:
        edit(states, placed)
    agent_state, agent_attr, agent_present = states[:, :A], attributes[:, :A], placed[:, :A]
    if agents is not None:
        agent_state = agents.to(DEV)
        agent_attr = attributes[:, :1].expand(B, agent_state.shape[1], 3)
        agent_present = torch.ones(agent_state.shape[:2], dtype=torch.bool, device=DEV)
    km = KinematicBicycle(dt=dt)
    km.set_params(lr=agent_attr[..., 2].contiguous())
    km.set_state(agent_state.contiguous())
    ctrl = LaneFollowingNPCController(lanes, attributes[:, A:, :2].contiguous(), states[:, A:].contiguous(), placed[:, A:].contiguous(), seed=seed + 1,
                                      **ctrl_kw)
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    return Simulator(BirdviewMesh.empty(batch_size=B).to(DEV), km, agent_attr[..., :2].contiguous(), agent_present.contiguous(), cfg, renderer=renderer,
                     npc_controller=ctrl, lanelet_map=lanes, traffic_controls=lights)


def snapshot(ctrl):
    return {k: getattr(ctrl, k).clone() for k in ('lane', 'arc', 'hops', 'leader', 'npc_state', 'npc_sc', 'npc_present_mask')}


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def within_one_ulp(got, want):
    return (got == want) | (got == np.nextafter(want, F32(np.inf))) | (got == np.nextafter(want, F32(-np.inf)))


def step_and_compare(sim, towns, which, action=None, what=''):
    """one Simulator.step, the NPC rows against the model; returns the model's per-scene outputs"""
    _, models = towns
    ctrl = sim.npc_controller
    B, N = ctrl.npc_state.shape[:2]
    A = sim.agent_count
    before = {k: v.cpu().numpy() for k, v in snapshot(ctrl).items()}
    boxes, sc, speed, present = (t.cpu().numpy() for t in ctrl._entities(sim))
    size, v0, ids = ctrl.npc_size.cpu().numpy(), ctrl.desired_speed.cpu().numpy(), ctrl.scene_ids.cpu().numpy()
    sim.step(torch.zeros((B, A, 2), device=DEV) if action is None else action)
    after = {k: v.cpu().numpy() for k, v in snapshot(ctrl).items()}
    outs = []
    for b in range(B):
        out = lf.step_scene(models[which[b]], before['lane'][b], before['arc'][b], before['hops'][b], before['npc_state'][b], size[b], v0[b],
                            before['npc_present_mask'][b], boxes[b], sc[b], speed[b], present[b], np.arange(A, A + N), ctrl.seed, int(ids[b]),
                            sim.kinematic_model.dt, ctrl.horizon, ctrl.lateral_margin, ctrl.idm)
        outs.append(out)
        tag = f'{what} scene {b}'
        for k in ('lane', 'hops', 'leader'):
            assert np.array_equal(after[k][b], out[k]), (tag, k, np.nonzero(after[k][b] != out[k])[0], after[k][b], out[k])
        assert np.array_equal(after['arc'][b], out['arc']), (tag, 'arc', np.abs(after['arc'][b] - out['arc']).max())
        got, want = after['npc_state'][b], out['state']
        for c, name in ((0, 'x'), (1, 'y'), (3, 'speed')):
            assert np.array_equal(got[:, c], want[:, c]), (tag, name, np.abs(got[:, c] - want[:, c]).max())
        assert within_one_ulp(got[:, 2], want[:, 2]).all(), (tag, 'psi')
        moved = out['moved']
        assert np.array_equal(after['npc_sc'][b][moved], out['sc'][moved]), (tag, '[sin, cos]')
        # rows that do not move are copied through: state and [sin, cos] exactly as they were
        assert np.array_equal(got[~moved], before['npc_state'][b][~moved]) and np.array_equal(after['npc_sc'][b][~moved], before['npc_sc'][b][~moved])
        assert (after['leader'][b][~moved] == -1).all()
    return outs


def check_snap(ctrl, towns, which, rows=None):
    """the constructor's one snap_to_lanes call against the model: lane and arc exactly"""
    from torchdrivesim_amd.lanelet2 import snap_to_lanes
    _, models = towns
    st = ctrl.npc_state
    lane, arc, lateral = (t.cpu().numpy() for t in snap_to_lanes(ctrl.lanelet_maps, st, ctrl.tolerance))
    assert np.array_equal(lane, ctrl.lane.cpu().numpy()) and np.array_equal(arc, ctrl.arc.cpu().numpy())
    xy, sc = st[..., :2].cpu().numpy(), torch.stack([torch.sin(st[..., 2]), torch.cos(st[..., 2])], -1).cpu().numpy()
    for b in range(st.shape[0]):
        for n in (range(st.shape[1]) if rows is None else rows):
            l, a, lat = lf.snap(models[which[b]], xy[b, n, 0], xy[b, n, 1], sc[b, n, 0], sc[b, n, 1], ctrl.tolerance)
            assert (lane[b, n], arc[b, n], lateral[b, n]) == (l, a, lat), (b, n, lane[b, n], arc[b, n], lateral[b, n], l, a, lat)


# ---------------------------------------------------------------------------------------------------------------- single steps
WHICH = [0, 1, 0, 1]
A4, N16 = 4, 16
STOP = (17.0, 0.5, 4.0)                  # stop lines: metres ahead of the NPC's start arc, thickness, width


def hand_placed(towns, dt_two=False, seed_for_routes=None):
    """the rows the issue names, per scene on its own long lanelets (NPC n is row A4 + n):
       NPC 0 with NPC 1 standing 6 m ahead; NPC 2 with agent 0 on the opposite side of the road beside its path; NPC 3 0.3 m before its lanelet's
       end; NPC 4 with agent 1 overlapping it; NPC 5 not present; NPC 6 off the map (lane -1); NPC 7 / 8 / 9 before a red / green / padded stop line.
       Every other agent or NPC within 45 m of one of these is taken out, so that the named rows meet what they are meant to meet."""
    _, models = towns
    spots = []

    def edit(states, present):
        for b, w in enumerate(WHICH):
            m = models[w]
            ll = long_lanelets(m)
            l3 = ll[2]
            if dt_two:      # a lanelet whose successor (as this NPC will choose it) is short enough to be crossed whole in one step of 2 s
                l3 = next(l for l in range(len(m)) if m.eligible(l) and m.succ[l] and
                          0 <= m.successor(l, seed_for_routes, b, 3, 0) and m.length(m.successor(l, seed_for_routes, b, 3, 0)) < 15.0)
            rows = {A4 + 0: pose_row(m, ll[0], 5.0, 6.0), A4 + 1: pose_row(m, ll[0], 11.0, 0.0),
                    A4 + 2: pose_row(m, ll[1], 5.0, 6.0), 0: pose_row(m, ll[1], 15.0, 5.0, left=3.6, reverse=True),
                    A4 + 3: pose_row(m, l3, m.length(l3) - 0.3, 8.0),
                    A4 + 4: pose_row(m, ll[3], 5.0, 3.0), 1: pose_row(m, ll[3], 6.0, 0.0),
                    A4 + 6: [5000.0, 5000.0, 0.3, 4.0],
                    A4 + 7: pose_row(m, ll[4], 5.0, 6.0), A4 + 8: pose_row(m, ll[5], 5.0, 6.0), A4 + 9: pose_row(m, ll[6], 5.0, 6.0)}
            named = torch.tensor([rows[k][:2] for k in rows if k != A4 + 6], device=DEV)
            near = (torch.cdist(states[b, :, :2], named) < 45.0).any(-1)
            present[b] &= ~near
            for k, row in rows.items():
                states[b, k] = torch.tensor(row, device=DEV)
                present[b, k] = True
            present[b, A4 + 5] = False
            spots.append([pose_row(m, ll[4 + i], 5.0 + STOP[0], 0.0) for i in range(3)])
    return edit, spots


def lights_for(spots):
    from torchdrivesim_amd.traffic_controls import TrafficLightControl
    pos = torch.tensor([[[x, y, STOP[1], STOP[2], psi] for x, y, psi, _ in scene] for scene in spots], dtype=torch.float32, device=DEV)
    mask = torch.tensor([[True, True, False]] * len(spots), device=DEV)
    lights = TrafficLightControl(pos, mask=mask)
    lights.set_state(torch.tensor([[0, 2, 0]] * len(spots), device=DEV))           # red, green, (padding) red
    return {'traffic_light': lights}


def test_single_steps_equal_the_model(towns):
    edit, spots = hand_placed(towns)
    sim = make_sim(towns, WHICH, A4, N16, seed=101, edit=edit)
    sim.traffic_controls = lights_for(spots)
    ctrl = sim.npc_controller
    check_snap(ctrl, towns, WHICH)
    assert (ctrl.lane[:, 6] == -1).all() and (ctrl.lane[:, [0, 1, 2, 3, 4, 7, 8, 9]] >= 0).all()
    ctrl.desired_speed[:, 10] = 0.0                     # set behind the constructor's back: such a row stands still
    ctrl.desired_speed[0, 11] = float('nan')
    E = A4 + N16
    for it in range(3):
        outs = step_and_compare(sim, towns, WHICH, what=f'step {it}')
        for b, out in enumerate(outs):
            leader = out['leader']
            if it == 0:
                assert leader[0] == A4 + 1, 'the car 6 m ahead is the leader'
                assert leader[2] != 0, 'a car beside the path, on the other side of the road, is nobody\'s leader'
                assert leader[4] == 1 and out['state'][4, 3] < F32(3.0), 'an overlapping entity is braked for as hard as the IDM brakes'
                assert leader[7] == E + 0, 'the red stop line stands on the path'
                assert leader[8] != E + 1 and leader[9] != E + 2, 'a green and a padded stop line do not'
            assert not out['moved'][5] and not out['moved'][6] and not out['moved'][10] and (b > 0 or not out['moved'][11])
    assert (ctrl.hops[:, 3] == 1).all(), 'the NPC 0.3 m before its lanelet\'s end is on the next one'


def test_steps_of_two_seconds_make_several_hops(towns):
    seed = 131
    edit, _ = hand_placed(towns, dt_two=True, seed_for_routes=seed + 1)
    sim = make_sim(towns, WHICH, A4, N16, seed=seed, edit=edit, dt=2.0)
    for it in range(2):
        step_and_compare(sim, towns, WHICH, what=f'dt = 2 s, step {it}')
        if it == 0:
            assert (sim.npc_controller.hops[:, 3] >= 2).all(), 'two lanelet ends are crossed in one step'


@pytest.mark.parametrize('A, N, extra, crowd', [(2, 1, 0, False), (4, 65, 0, False), (65, 65, 0, False), (4, 65, 411, False), (4, 65, 412, False), (4, 65, 456, False),
                                                 (4, 65, 200, True)], ids=['N1', 'N65', 'E130', 'E480', 'E481', 'E525', 'crowd'])
def test_shapes(towns, A, N, extra, crowd):
    """one NPC; more NPCs than one workgroup column; E = 130; E = 480, the last size with four NPCs per workgroup and exactly 64 KiB of LDS, E = 481 and 525, where a workgroup holds two -- the extra
    entities are agents scattered around the NPCs, off the lanes or on them; a crowd of 204 agents within 10 m of ONE NPC, more in reach of its
    path than the 64 the kernel keeps before it weighs them"""
    which = [0, 1]
    agents = None
    if extra:
        base = make_sim(towns, which, A, N, seed=7 + N)
        g = torch.Generator(device='cpu').manual_seed(5)
        npc = base.npc_controller.npc_state.cpu()
        pick = torch.randint(0, N, (2, A + extra), generator=g) * (0 if crowd else 1)
        agents = torch.gather(npc, 1, pick[..., None].expand(-1, -1, 4)).clone()
        agents[..., :2] += (torch.rand(2, A + extra, 2, generator=g) - 0.5) * (20.0 if crowd else 60.0)
        agents[..., 2] += (torch.rand(2, A + extra, generator=g) - 0.5) * 1.0
    sim = make_sim(towns, which, A, N, seed=7 + N, agents=agents)
    assert sim.agent_count + N == A + extra + N
    check_snap(sim.npc_controller, towns, which, rows=range(min(N, 6)))
    for it in range(1 if extra else 2):
        outs = step_and_compare(sim, towns, which, what=f'A {A} N {N} step {it}')
    if extra and not crowd:
        assert sum(int((o['leader'] >= 0).sum()) for o in outs) >= 10, 'the scattered agents are in the way of some NPCs'
    if crowd:
        assert all(0 <= o['leader'][0] < A + extra for o in outs), 'NPC 0 stands in a crowd'


# ---------------------------------------------------------------------------------------------------------------- rollout
def test_a_rollout_of_100_steps_stays_on_the_model(towns):
    """B = 2 scenes x N = 32 NPCs on Town01, every step held to the bar; desired speeds of 5 and 11 m/s by turns, so that by the end NPCs have
    changed lanelets and the fast have caught up with the slow"""
    v0 = torch.tensor([5.0, 11.0], device=DEV).repeat(16)[None].expand(2, 32)
    sim = make_sim(towns, [0, 0], 2, 32, seed=211, desired_speed=v0)
    hops0 = sim.npc_controller.hops.clone()
    led = 0
    for it in range(100):
        outs = step_and_compare(sim, towns, [0, 0], what=f'rollout step {it}')
        led += sum(int((o['leader'] >= 0).sum()) for o in outs)
    ctrl = sim.npc_controller
    print('rollout: hops', int((ctrl.hops - hops0).sum()), 'NPC-steps behind a leader', led)
    assert int((ctrl.hops - hops0).sum()) >= 32 and led > 0
    assert bool((ctrl.npc_state[..., 3] > 1.0).any())


# ---------------------------------------------------------------------------------------------------------------- batch plumbing
def test_batch_operations_reproduce_the_rows_bit_for_bit(towns):
    from torchdrivesim_amd.parallel import shard_simulator
    which = [0, 1, 1, 0, 0, 1]
    B, A, N, steps = len(which), 2, 8, 4
    sim = make_sim(towns, which, A, N, seed=307)
    idx = [4, 0, 3]
    variants = {'select': (sim.select_batch_elements(idx, in_place=False), idx), 'copy': (sim.copy(), list(range(B))),
                'extend': (sim.extend(2, in_place=False), [b for b in range(B) for _ in range(2)]),
                'shard 0': (shard_simulator(sim, 0, 2), [0, 1, 2]), 'shard 1': (shard_simulator(sim, 1, 2), [3, 4, 5])}
    # the same scenes 2 and 5 set up on their own, told which scenes of the stream they are
    alone = make_sim(towns, which, A, N, seed=307).select_batch_elements([2, 5], in_place=False)
    assert torch.equal(alone.npc_controller.scene_ids, torch.tensor([2, 5], device=DEV))
    from torchdrivesim_amd.behavior.lane_follow import LaneFollowingNPCController
    c = alone.npc_controller
    alone.npc_controller = LaneFollowingNPCController([c.lanelet_maps[0], c.lanelet_maps[1]], c.npc_size, c.npc_state, c.npc_present_mask, seed=c.seed,
                                                      scene_ids=torch.tensor([2, 5], device=DEV))
    variants['explicit scene_ids'] = (alone, [2, 5])
    g = torch.Generator(device='cpu').manual_seed(1)
    actions = (torch.rand(steps, B, A, 2, generator=g) * 2 - 1).to(DEV)
    for t in range(steps):
        sim.step(actions[t])
        for other, rows in variants.values():
            other.step(actions[t][rows])
    whole = snapshot(sim.npc_controller)
    for name, (other, rows) in variants.items():
        part = snapshot(other.npc_controller)
        for k in whole:
            assert torch.equal(part[k], whole[k][rows]), (name, k)
    # and the copies did not share a buffer with the original
    before = snapshot(sim.npc_controller)
    variants['copy'][0].step(actions[0])
    assert same(snapshot(sim.npc_controller), before)


# ---------------------------------------------------------------------------------------------------------------- graph capture
def test_a_captured_step_replays_the_eager_bits(towns):
    which = [0, 1] * 4
    B, A, N = len(which), 4, 16
    sim, ref = (make_sim(towns, which, A, N, seed=401) for _ in range(2))
    g0 = torch.Generator(device='cpu').manual_seed(3)
    actions = (torch.rand(10, B, A, 2, generator=g0) * 2 - 1).to(DEV)
    state = sim.get_state().clone()
    action = actions[0].clone()
    start = snapshot(sim.npc_controller)

    def step():
        sim.kinematic_model.set_state(state)
        sim.step(action)
        return sim.get_state()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()                                          # warm-up: lane tables, the self-index rows
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ctrl = sim.npc_controller
    for k, v in start.items():                              # back to the start: the controller's buffers are written in place
        getattr(ctrl, k).copy_(v)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        new = step()
        state_next = new.clone()
    for k, v in start.items():                              # capturing runs nothing, but be explicit
        getattr(ctrl, k).copy_(v)
    for i in range(10):
        ref.step(actions[i])
        action.copy_(actions[i])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(new, ref.get_state()) and same(snapshot(ctrl), snapshot(ref.npc_controller)), f'replay {i}'
        state.copy_(state_next)
    assert bool((ctrl.arc != start['arc']).any())


# ---------------------------------------------------------------------------------------------------------------- traffic lights
def test_an_npc_waits_at_a_red_light_and_goes_on_green(towns):
    """Town01's own stop lines (tests/golden/maps): an NPC 25 m before a traffic light's stop line comes to rest in front of it while the light is
    red and drives on once it is green.  On `revert_map` of the town: the package's stop lines lie at the END of the reverted lanelets -- the
    file stores its lanelets against the direction of travel ("Wrong-way")."""
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.map import load_map_config, traffic_controls_from_map_config
    reverted = lanelet2.revert_map(towns[0][0])
    m = lf.Lanes(reverted)
    towns = ([reverted], [m])
    cfg = load_map_config(os.path.join(GOLDEN, 'maps', 'carla_Town01', 'metadata.json'))
    lights = traffic_controls_from_map_config(cfg)['traffic_light'].to(DEV)
    pos = lights.pos[0].cpu().numpy()
    found = None
    for k, (x, y) in enumerate(pos[:, :2]):
        for l in range(len(m)):
            if not m.eligible(l) or m.length(l) < 30.0:
                continue
            kk, u, tx, ty = lf.foot(m.cl[l], float(x), float(y))
            fx, fy = m.cl[l][kk][0] + u * (m.cl[l][kk + 1][0] - m.cl[l][kk][0]), m.cl[l][kk][1] + u * (m.cl[l][kk + 1][1] - m.cl[l][kk][1])
            arc = m.cum[l][kk] + u * (m.cum[l][kk + 1] - m.cum[l][kk])
            if math.hypot(fx - x, fy - y) < 0.5 and arc > 27.0:
                found = (k, l, arc)
                break
        if found:
            break
    assert found, 'no stop line of a traffic light lies on a centre line 27 m into a lanelet'
    k, l, stop_arc = found
    length = 4.97

    def edit(states, present):
        states[0, 1] = torch.tensor(pose_row(m, l, stop_arc - 25.0, 8.0), device=DEV)
        states[0, 0] = torch.tensor([5000.0, 5000.0, 0.0, 0.0], device=DEV)
    sim = make_sim(towns, [0], 1, 1, seed=503, edit=edit)
    sim.traffic_controls = {'traffic_light': lights}
    ctrl = sim.npc_controller
    assert ctrl.lane[0, 0].item() == l
    red, green = lights.allowed_states.index('red'), lights.allowed_states.index('green')
    lights.set_state(torch.full_like(lights.state, red))
    zero = torch.zeros((1, 1, 2), device=DEV)
    for _ in range(150):
        sim.step(zero)
    front = ctrl.arc[0, 0].item() + length / 2
    near_edge = stop_arc - float(pos[k, 2]) / 2
    assert ctrl.npc_state[0, 0, 3].item() == 0.0 and ctrl.lane[0, 0].item() == l and ctrl.leader[0, 0].item() == 1 + 1 + k
    assert near_edge - 3.0 <= front <= near_edge, (front, near_edge)
    lights.set_state(torch.full_like(lights.state, green))
    for _ in range(60):
        sim.step(zero)
    assert ctrl.npc_state[0, 0, 3].item() > 3.0 and (ctrl.hops[0, 0].item() > 0 or ctrl.arc[0, 0].item() > stop_arc + 2.0)
    # with obey_traffic_lights=False the red light is not there
    sim2 = make_sim(towns, [0], 1, 1, seed=503, edit=edit, obey_traffic_lights=False)
    sim2.traffic_controls = {'traffic_light': lights}
    lights.set_state(torch.full_like(lights.state, red))
    for _ in range(60):
        sim2.step(zero)
    assert sim2.npc_controller.npc_state[0, 0, 3].item() > 3.0


# ---------------------------------------------------------------------------------------------------------------- compound controller
def test_a_compound_of_replay_and_lane_following_advances_both(towns):
    from torchdrivesim_amd.behavior import ReplayController
    from torchdrivesim_amd.simulator import CompoundNPCController
    which = [0, 1]
    B, A, N, T = 2, 2, 6, 5
    sim = make_sim(towns, which, A, N, seed=601)
    follow = sim.npc_controller
    log = follow.npc_state.clone()[:, :, None, :].repeat(1, 1, T, 1)
    log[..., 0] += torch.arange(T, device=DEV)[None, None, :] * 0.5                  # the replayed NPCs slide 0.5 m per frame
    replay = ReplayController(follow.npc_size, log)
    owner = torch.tensor([[0, 0, 1, 1, 1, 1]] * B, device=DEV)                        # NPCs 0, 1 are replayed, 2 .. 5 follow their lanes
    sim.npc_controller = CompoundNPCController([replay, follow], owner)
    start = sim.get_npc_state().clone()
    mine = snapshot(follow)
    for t in range(1, 4):
        sim.step(torch.zeros((B, A, 2), device=DEV))
        now = sim.get_npc_state()
        assert torch.equal(now[:, :2], log[:, :2, t])
        assert bool((now[:, 2:, :2] != start[:, 2:, :2]).any(-1).all()), 'the lane-following NPCs move'
    assert bool(((follow.arc[:, 2:] > mine['arc'][:, 2:]) | (follow.hops[:, 2:] > 0)).all())


def test_a_standing_sibling_in_a_compound_stays_put(towns):
    """a base NPCController keeps the tensor the compound hands to all members: the lane-following member must not write into it, and must
    move its own rows only"""
    from torchdrivesim_amd.simulator import CompoundNPCController, NPCController
    which = [0, 1]
    B, A, N = 2, 2, 6
    sim = make_sim(towns, which, A, N, seed=611)
    follow = sim.npc_controller
    parked = NPCController(follow.npc_size.clone(), follow.npc_state.clone(), follow.npc_present_mask.clone())
    owner = torch.tensor([[0, 1, 0, 1, 1, 0]] * B, device=DEV)
    sim.npc_controller = CompoundNPCController([parked, follow], owner)
    start = sim.get_npc_state().clone()
    for _ in range(5):
        sim.step(torch.zeros((B, A, 2), device=DEV))
    now = sim.get_npc_state()
    mine = owner == 1
    assert torch.equal(now[~mine], start[~mine]), 'the parked NPCs were moved'
    assert bool((now[mine][:, :2] != start[mine][:, :2]).any(-1).all())
    assert bool((follow.leader[~mine] == -1).all())


def test_two_lane_following_members_equal_one(towns):
    """a compound of two lane-following controllers that own half the NPCs each is the single controller bit for bit: every member reads the
    scene as it was before the step, whichever advances first"""
    from torchdrivesim_amd.simulator import CompoundNPCController
    which = [0, 1, 0]
    B, A, N = 3, 2, 12
    one, two = (make_sim(towns, which, A, N, seed=613) for _ in range(2))
    first = two.npc_controller
    second = first.copy()
    owner = (torch.arange(N, device=DEV) % 2)[None].expand(B, N).contiguous()
    two.npc_controller = CompoundNPCController([first, second], owner)
    g = torch.Generator(device='cpu').manual_seed(2)
    for _ in range(6):
        action = (torch.rand(B, A, 2, generator=g) * 2 - 1).to(DEV)
        one.step(action)
        two.step(action)
        assert torch.equal(two.get_npc_state(), one.get_npc_state())
    ref = one.npc_controller
    for member, rows in ((first, owner == 0), (second, owner == 1)):
        for k in ('lane', 'arc', 'hops', 'leader'):
            assert torch.equal(getattr(member, k)[rows], getattr(ref, k)[rows]), k


def test_a_spawned_npc_starts_from_the_lane_under_its_new_pose(towns):
    from torchdrivesim_amd.simulator import SpawnController
    _, models = towns
    m = models[0]
    ll = long_lanelets(m)
    T, at = 8, 2

    def edit(states, present):
        states[0, 1] = torch.tensor(pose_row(m, ll[0], 20.0, 5.0), device=DEV)
        states[0, 2] = torch.tensor(pose_row(m, ll[2], 20.0, 5.0), device=DEV)
        present[0, 2] = False
    sim = make_sim(towns, [0], 1, 2, seed=617, edit=edit)
    ctrl = sim.npc_controller
    pose = torch.tensor(pose_row(m, ll[4], 50.0, 5.0), device=DEV)
    spawn_states = torch.zeros((1, 2, T, 4), device=DEV)
    spawn_states[0, 1, at] = pose
    spawn_masks = torch.zeros((1, 2, T), dtype=torch.bool, device=DEV)
    spawn_masks[0, 1, at] = True
    ctrl.spawn_controller = SpawnController(spawn_states=spawn_states, spawn_masks=spawn_masks)
    zero = torch.zeros((1, 1, 2), device=DEV)
    for _ in range(at + 1):
        sim.step(zero)
    assert bool(ctrl.npc_present_mask[0, 1]) and torch.equal(ctrl.npc_state[0, 1], pose)
    assert ctrl.lane[0, 1].item() == ll[4] and abs(ctrl.arc[0, 1].item() - 50.0) < 1e-3 and ctrl.hops[0, 1].item() == 0
    step_and_compare(sim, towns, [0], what='the step after the spawn')
    assert ctrl.lane[0, 1].item() == ll[4] and 50.3 < ctrl.arc[0, 1].item() < 50.7
    assert float((ctrl.npc_state[0, 1, :2] - pose[:2]).norm()) < 1.0, 'the spawned NPC jumped back to where its row was before'
    assert ctrl.lane[0, 0].item() == ll[0] and ctrl.arc[0, 0].item() > 21.0          # the row that was there all along went on as it was


# ---------------------------------------------------------------------------------------------------------------- single-map entry points
def test_the_single_map_forms_equal_the_set_forms(towns):
    """tds_lane_snap and tds_lane_follow_step take one lane table where the _multi forms take a set: the same kernels, the same bits"""
    import ctypes
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import LANELET_TAGS_TO_EXCLUDE
    maps, _ = towns
    sim = make_sim(towns, [0, 0, 0], 3, 9, seed=809)
    ctrl = sim.npc_controller
    B, N = ctrl.npc_state.shape[:2]
    table = maps[0].table(DEV, LANELET_TAGS_TO_EXCLUDE)
    dev = torch.device(DEV)
    f64, i32, f32 = torch.float64, torch.int32, torch.float32
    xy, sc = ctrl.npc_state[..., :2].contiguous(), _ops.heading_sc(ctrl.npc_state[..., 2])
    lane, arc, lateral = torch.empty((B, N), dtype=i32, device=dev), torch.empty((B, N), dtype=f64, device=dev), torch.empty((B, N), dtype=f32, device=dev)
    nat.call('tds_lane_snap', dev, table.handle, nat.dev_ptr(xy, f32, 'xy'), nat.dev_ptr(sc, f32, 'sc'), nat.dev_ptr(lane, i32, 'lane'),
             nat.dev_ptr(arc, f64, 'arc'), nat.dev_ptr(lateral, f32, 'lateral'), B * N, 1.0, nat.stream_ptr(dev))
    want = _ops.lane_snap(ctrl._lane_table_set(), xy, sc, 1.0)
    assert torch.equal(lane, want[0]) and torch.equal(arc, want[1]) and torch.equal(lateral, want[2]) and bool((lane >= 0).all())
    boxes, esc, speed, present = ctrl._entities(sim)
    E = boxes.shape[1]
    mine = snapshot(ctrl)
    self_index = torch.arange(3, 3 + N, dtype=i32, device=dev).expand(B, N).contiguous()
    idm = (ctypes.c_float * 5)(*ctrl.idm)
    u8 = lambda t: ctypes.c_void_p(t.contiguous().view(torch.uint8).data_ptr())
    nat.call('tds_lane_follow_step', dev, table.handle, nat.dev_ptr(ctrl.scene_ids, torch.int64, 'ids'), B, N, E, nat.dev_ptr(boxes.contiguous(), f32, 'boxes'),
             nat.dev_ptr(esc.contiguous(), f32, 'sc'), nat.dev_ptr(speed, f32, 'speed'), u8(present), nat.dev_ptr(self_index, i32, 'self'),
             nat.dev_ptr(ctrl.npc_size.contiguous(), f32, 'size'), nat.dev_ptr(ctrl.desired_speed, f32, 'v0'), u8(ctrl.npc_present_mask),
             nat.dev_ptr(mine['lane'], i32, 'lane'), nat.dev_ptr(mine['arc'], f64, 'arc'), nat.dev_ptr(mine['hops'], i32, 'hops'),
             nat.dev_ptr(mine['npc_state'], f32, 'state'), nat.dev_ptr(mine['npc_sc'], f32, 'npc_sc'), nat.dev_ptr(mine['leader'], i32, 'leader'),
             ctrl.seed, 0.1, ctrl.horizon, ctrl.lateral_margin, ctypes.cast(idm, ctypes.c_void_p), nat.stream_ptr(dev))
    ctrl.advance_npcs(sim)
    assert same(mine, snapshot(ctrl)) and bool((mine['arc'] != arc).any())


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_come_before_any_launch(towns):
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.behavior.lane_follow import LaneFollowingNPCController
    from torchdrivesim_amd.lanelet2 import snap_to_lanes
    maps, _ = towns
    sim = make_sim(towns, [0], 2, 3, seed=701)
    ctrl = sim.npc_controller
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        LaneFollowingNPCController(maps[0], ctrl.npc_size.cpu(), ctrl.npc_state.cpu(), seed=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        snap_to_lanes(maps[0], ctrl.npc_state.cpu())
    before = snapshot(ctrl)
    sim.kinematic_model.dt = -0.1
    with pytest.raises(nat.TdsError) as e:
        ctrl.advance_npcs(sim)
    assert e.value.code == nat.E_INVAL and 'dt' in str(e.value)
    sim.kinematic_model.dt = 0.1
    with pytest.raises(nat.TdsError) as e:
        LaneFollowingNPCController(maps[0], ctrl.npc_size, ctrl.npc_state, seed=1, idm=(1.5, 2.0, float('nan'), 2.0, 6.0))
    assert e.value.code == nat.E_INVAL
    with pytest.raises(ValueError, match='desired_speed'):
        LaneFollowingNPCController(maps[0], ctrl.npc_size, ctrl.npc_state, seed=1, desired_speed=0.0)
    # more entities than a scene's LDS holds: refused by the wrapper and by the entry point itself, TDS_ELIMIT both
    E = nat.FOLLOW_MAX_ENTITIES + 1
    boxes = torch.zeros((1, E, 5), device=DEV)
    args = (ctrl._lane_table_set(), ctrl.scene_ids, boxes, torch.zeros((1, E, 2), device=DEV), torch.zeros((1, E), device=DEV),
            torch.zeros((1, E), dtype=torch.bool, device=DEV), None, ctrl.npc_size, ctrl.desired_speed, ctrl.npc_present_mask, ctrl.lane, ctrl.arc,
            ctrl.hops, ctrl.npc_state, ctrl.npc_sc, ctrl.leader, 1, 0.1)
    with pytest.raises(nat.TdsError) as e:
        _ops.lane_follow_step(*args)
    assert e.value.code == nat.E_LIMIT
    idm = np.ones(5, np.float32)
    rc = nat.lib().tds_lane_follow_step_multi(ctrl._lane_table_set().handle, None, None, 1, 3, E, *([None] * 14), 1, 0.1, 60.0, 0.2,
                                              idm.ctypes.data, None)
    assert rc == nat.E_LIMIT and 'entities' in nat.last_error()
    rc = nat.lib().tds_lane_follow_step_multi(ctrl._lane_table_set().handle, None, None, 1, 3, 4, *([None] * 14), 1, -0.1, 60.0, 0.2,
                                              idm.ctypes.data, None)
    assert rc == nat.E_INVAL and 'dt' in nat.last_error()
    torch.cuda.synchronize()
    assert same(snapshot(ctrl), before), 'a refused call wrote nothing'
