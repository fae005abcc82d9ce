#!/usr/bin/env python3
"""
The loop of the reference's examples/gym_env.py:83-126 (GymEnv.step) on this framework: act -> Simulator.step -> bird's-eye observation ->
infractions as reward terms.  Runs on one MI355X with the Town01 package shipped under tests/golden/ (mesh, stop lines, light programmes,
lane map); the "policy" is random.

    python examples/step_loop.py [--batch 64] [--agents 16] [--steps 50] [--res 128]
    python examples/step_loop.py --scan 64          # a non-visual loop: 64-ray range scans (other agents, road edge) instead of images
    python examples/step_loop.py --scan 64 --scan-grad   # one step: a keep-clear-of-the-road-edge penalty on the scan, differentiated to the actions
    python examples/step_loop.py --neighbors 8      # a non-visual loop: the 8 nearest other agents in each agent's frame, with their relative velocity
    python examples/step_loop.py --ttc 5            # beside whatever is observed: when each agent would first hit another one within 5 s at constant velocity
    python examples/step_loop.py --lanes 6          # a non-visual loop: the 6 nearest lanes in each agent's frame, each a foot point and a polyline ahead
    python examples/step_loop.py --lights device --stop-lines 4     # the light programmes run on the device, a clock per scene; a non-visual loop sees
                                                                    # the 4 nearest stop lines ahead with their colour and the seconds until it changes
    python examples/step_loop.py --npcs 32          # 32 NPCs per scene that follow the lanes (IDM), stop at red lights and for the agents
    python examples/step_loop.py --npcs 32 --give-way       # ... and give way to each other at junctions (a second launch per step)
    python examples/step_loop.py --route 200        # every agent gets a 200 m route on the lane graph: progress as a reward term, lookahead as observation
    python examples/step_loop.py --route-to         # every agent gets the shortest route to a random on-lane destination, planned again when it strays
    python examples/step_loop.py --route-grad       # a few steps of gradient descent on the actions through the simulator, with a route loss
    python examples/step_loop.py --ttc-grad         # one step: a time-to-collision penalty differentiated to the actions through the simulator
    python examples/step_loop.py --neighbors-grad   # one step: a keep-your-distance penalty on the neighbour features differentiated to the actions
    python examples/step_loop.py --lanes 6 --lanes-grad     # one step: a lane-keeping penalty on the lane features differentiated to the actions
    python examples/step_loop.py --lights device --stop-lines 4 --stop-lines-grad   # one step: a do-not-cross-the-red-line penalty differentiated to the actions
    python examples/step_loop.py --wrong-way-grad   # one step: the wrong-way loss differentiated to the actions (it reaches them through psi alone)
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (scene construction shared with the benchmark)
from torchdrivesim_amd import lanelet2  # noqa: E402
from torchdrivesim_amd.map import load_map_config, programmed_traffic_lights_from_map_config, traffic_controls_from_map_config  # noqa: E402
from torchdrivesim_amd.traffic_lights import current_light_state_tensor_from_controller  # noqa: E402
from torchdrivesim_amd.utils import Resolution  # noqa: E402


def route_grad_loop(args, sim, lanes, dev):
    """--route-grad: "get somewhere" by backpropagation.  Every agent is dealt a route with differentiable=True; each step the actions are applied,
    the route loss of the state they lead to is differentiated to them through the kinematic step (one backward launch for the route step, one for
    the kinematics), and they take a gradient step.  No policy, no images: the loop only shows the task term of a loss reaching the actions."""
    from torchdrivesim_amd.goals import RouteGoal
    sim.route_goals = RouteGoal.sample(lanelet2.revert_map(lanes), sim.get_state(), sim.get_present_mask(), seed=2, length=args.route or 200.0,
                                       differentiable=True)
    valid = sim.route_goals.valid
    action = torch.zeros((args.batch, args.agents, 2), device=dev, requires_grad=True)
    steps = min(args.steps, 20)
    for it in range(steps):
        sim.kinematic_model.set_state(sim.get_state().detach())             # each step differentiates through itself alone
        sim.step(action)
        route = sim.compute_route_progress()                               # float fields with the graph; the flags are plain buffers
        # advance differentiates as progress (the stored progress is a constant); stay on the route's line and along it
        loss = -route.advance.sum() + 0.1 * (route.lateral ** 2).sum() + (route.heading[..., 0] ** 2).sum()
        grad, = torch.autograd.grad(loss, action)
        with torch.no_grad():
            action.sub_(0.5 * grad).clamp_(-1.0, 1.0)
        if it in (0, steps - 1):
            n = valid.sum().clamp(min=1)
            print(f'step {it}: advance {float(route.advance.detach().sum() / n):.3f} m, |lateral| {float(route.lateral.detach().abs().sum() / n):.3f} m per routed agent, '
                  f'|d loss / d action| {float(grad.abs().mean()):.4f}, mean acceleration command {float(action[..., 0].mean()):+.3f}')


def ttc_grad_step(args, sim, dev):
    """--ttc-grad: "do not be on course to overlap" by backpropagation.  One step: the actions are applied, every agent with a finite time to
    collision within the horizon pays (horizon - ttc).clamp(min=0), and that penalty is differentiated to the actions through the backward launch of
    time to collision and the kinematic step.  compute_collision() has no gradient for these agents: nothing overlaps yet."""
    horizon = args.ttc or 5.0
    action = torch.zeros((args.batch, args.agents, 2), device=dev, requires_grad=True)
    sim.kinematic_model.set_state(sim.get_state().detach())
    sim.step(action)
    first = sim.compute_time_to_collision(k=1, horizon=horizon, differentiable=True).min      # (B, A) seconds, with the graph
    finite = torch.isfinite(first)
    penalty = torch.where(finite, (horizon - first).clamp(min=0), torch.zeros_like(first)).sum()
    grad, = torch.autograd.grad(penalty, action)
    on_course = finite & (first.detach() > 0)
    print(f'{int(finite.sum())} of {finite.numel()} agents have a time to collision within {horizon:g} s ({int(on_course.sum())} not overlapping yet), penalty '
          f'{float(penalty.detach()):.2f} s; |d penalty / d action| {float(grad.abs().sum(-1)[on_course].mean()) if bool(on_course.any()) else 0.0:.4f} on '
          f'average over those agents, {int((grad.abs().sum(-1) > 0).sum())} agents with a gradient')


def neighbors_grad_step(args, sim, dev):
    """--neighbors-grad: the observation of a vector policy with its gradient.  One step: the actions are applied, every agent pays
    (comfort - distance).clamp(min=0) for each of its K nearest neighbours closer than `comfort` metres plus a little for a closing speed, and that
    penalty is differentiated to the actions through the backward launch of the neighbour observations and the kinematic step -- to the observer's
    action and to the neighbour's."""
    k, comfort = args.neighbors or 8, 15.0
    action = torch.zeros((args.batch, args.agents, 2), device=dev, requires_grad=True)
    sim.kinematic_model.set_state(sim.get_state().detach())
    sim.step(action)
    near = sim.compute_neighbors(k=k, max_distance=args.scan_range, differentiable=True)      # features (B, A, K, 8) with the graph, index without
    x, y, vx = near.features[..., 0], near.features[..., 1], near.features[..., 4]
    distance = (x * x + y * y + 1e-6).sqrt()
    close = near.mask & (distance.detach() < comfort)                                         # an empty slot holds zeros: mask it, it is no neighbour at 0 m
    penalty = torch.where(close, (comfort - distance).clamp(min=0) + 0.1 * (-vx * x / distance).clamp(min=0), torch.zeros_like(distance)).sum()
    grad, = torch.autograd.grad(penalty, action)
    involved = close.any(-1)
    print(f'{int(near.mask.sum())} of {near.mask.numel()} neighbour slots filled within {args.scan_range:g} m, {int(close.sum())} closer than {comfort:g} m, penalty '
          f'{float(penalty.detach()):.2f}; |d penalty / d action| {float(grad.abs().sum(-1)[involved].mean()) if bool(involved.any()) else 0.0:.4f} on average '
          f'over the {int(involved.sum())} agents with such a neighbour, {int((grad.abs().sum(-1) > 0).sum())} agents with a gradient')


def lanes_grad_step(args, sim, dev):
    """--lanes-grad: the map half of a vector policy's observation with its gradient.  One step: the actions are applied, every agent pays
    lateral^2 + sin_rel^2 of the nearest lane that runs its way (cos_rel > 0) -- "stay centred, face along the lane" -- and that penalty is
    differentiated to the actions through the backward launch of the lane observations and the kinematic step.  The map is constant, so an
    agent's penalty reaches its own action alone."""
    k = args.lanes or 6
    action = torch.zeros((args.batch, args.agents, 2), device=dev, requires_grad=True)
    sim.kinematic_model.set_state(sim.get_state().detach())
    sim.step(action)
    lanes = sim.compute_lanes(k=k, differentiable=True)                   # features and points with the graph, n_valid and index without
    lateral, sin_rel, cos_rel = lanes.features[..., 6], lanes.features[..., 2], lanes.features[..., 3]
    along = lanes.mask & (cos_rel.detach() > 0)                           # an empty slot holds zeros: mask it, it is no lane at 0 m
    first = along & (along.cumsum(-1) == 1)                               # the nearest such lane: the slots are nearest first
    penalty = torch.where(first, lateral * lateral + sin_rel * sin_rel, torch.zeros_like(lateral)).sum()
    grad, = torch.autograd.grad(penalty, action)
    on_lane = first.any(-1)
    print(f'{int(lanes.mask.sum())} of {lanes.mask.numel()} lane slots filled, {int(on_lane.sum())} of {on_lane.numel()} agents with a lane that runs their way, '
          f'penalty {float(penalty.detach()):.2f}; |d penalty / d action| {float(grad.abs().sum(-1)[on_lane].mean()) if bool(on_lane.any()) else 0.0:.4f} on '
          f'average over those agents, {int((grad.abs().sum(-1) > 0).sum())} agents with a gradient')


def scan_grad_step(args, sim, dev):
    """--scan-grad: the lidar-like observation with its gradient.  One step: the actions are applied, every agent pays (clear - road).clamp(min=0)
    for each of its rays whose stretch of road ends less than `clear` metres away -- "keep clear of the road edge", a signal that is there long
    before compute_offroad() is non-zero -- and that penalty is differentiated to the actions through the backward launch of the range scans
    and the kinematic step.  The map is constant, so an agent's penalty reaches its own action alone."""
    rays, clear = args.scan or 64, 4.0
    action = torch.zeros((args.batch, args.agents, 2), device=dev, requires_grad=True)
    sim.kinematic_model.set_state(sim.get_state().detach())
    sim.step(action)
    scan = sim.compute_range_scan(n_rays=rays, max_range=args.scan_range, agents=False, differentiable=True)      # road with the graph, hit without
    near = (scan.road.detach() > 0) & (scan.road.detach() < clear)                          # 0: the agent is off the road already, the scan says nothing
    penalty = torch.where(near, (clear - scan.road).clamp(min=0), torch.zeros_like(scan.road)).sum()
    grad, = torch.autograd.grad(penalty, action)
    involved = near.any(-1)
    print(f'{int(near.sum())} of {near.numel()} rays leave the road within {clear:g} m, penalty {float(penalty.detach()):.2f} m; |d penalty / d action| '
          f'{float(grad.abs().sum(-1)[involved].mean()) if bool(involved.any()) else 0.0:.4f} on average over the {int(involved.sum())} agents with such a '
          f'ray, {int((grad.abs().sum(-1) > 0).sum())} agents with a gradient')


def stop_lines_grad_step(args, sim, dev):
    """--stop-lines-grad: the traffic-rule half of a vector policy's observation with its gradient.  One step: the actions are applied, every
    agent whose nearest stop line ahead shows red pays (brake - distance).clamp(min=0) + (brake - x).clamp(min=0) for coming within `brake` metres
    of it -- "do not cross the red line" -- and that penalty is differentiated to the actions through the backward launch of the stop-line
    observations and the kinematic step.  The lines are constants, so an agent's penalty reaches its own action alone."""
    k, brake = args.stop_lines or 4, 15.0
    action = torch.zeros((args.batch, args.agents, 2), device=dev, requires_grad=True)
    sim.kinematic_model.set_state(sim.get_state().detach())
    sim.step(action)
    lines = sim.compute_stop_lines(k=k, max_distance=args.scan_range, differentiable=True)      # features with the graph, index and state without
    x, distance = lines.features[:, :, 0, 0], lines.features[:, :, 0, 7]                        # slot 0: the nearest line ahead
    red = lines.mask[:, :, 0] & (lines.state[:, :, 0] == 0)                                     # an empty slot holds zeros: mask it, it is no line at 0 m
    near = red & (distance.detach() < brake)
    penalty = torch.where(near, (brake - distance).clamp(min=0) + (brake - x).clamp(min=0), torch.zeros_like(x)).sum()
    grad, = torch.autograd.grad(penalty, action)
    print(f'{int(lines.mask[:, :, 0].sum())} of {near.numel()} agents have a stop line ahead within {args.scan_range:g} m, {int(red.sum())} of them red, '
          f'{int(near.sum())} within {brake:g} m, penalty {float(penalty.detach()):.2f} m; |d penalty / d action| '
          f'{float(grad.abs().sum(-1)[near].mean()) if bool(near.any()) else 0.0:.4f} on average over those agents, '
          f'{int((grad.abs().sum(-1) > 0).sum())} agents with a gradient')


def wrong_way_grad_step(args, sim, dev):
    """--wrong-way-grad: the wrong-way term of the reward with its gradient.  One step: the actions are applied and compute_wrong_way's loss is
    differentiated to them.  As in the reference the position is a constant of this loss: the gradient reaches the actions through psi alone --
    through the steering, which turns the car round."""
    action = torch.zeros((args.batch, args.agents, 2), device=dev, requires_grad=True)
    sim.kinematic_model.set_state(sim.get_state().detach())
    sim.step(action)
    loss = sim.compute_wrong_way(differentiable=True)                     # (B, A) with the graph to psi
    grad, = torch.autograd.grad(loss.sum(), action)
    wrong = loss.detach() > 0
    print(f'{int(wrong.sum())} of {wrong.numel()} agents drive against their lane, loss {float(loss.detach().sum()):.2f}; |d loss / d steering| '
          f'{float(grad[..., 1].abs()[wrong].mean()) if bool(wrong.any()) else 0.0:.4f} on average over those agents, '
          f'{int((grad.abs().sum(-1) > 0).sum())} agents with a gradient')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--agents', type=int, default=16)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--scan', type=int, default=0, metavar='RAYS', help='observe RAYS-ray range scans (compute_range_scan) instead of images')
    ap.add_argument('--scan-range', type=float, default=50.0)
    ap.add_argument('--neighbors', type=int, default=0, metavar='K', help='observe the K nearest other agents (compute_neighbors) instead of images')
    ap.add_argument('--ttc', type=float, default=0.0, metavar='SECONDS', help='also compute every agent\'s time to collision within SECONDS each step '
                    '(compute_time_to_collision): an anticipatory safety term of a reward, beside whatever is observed')
    ap.add_argument('--lights', choices=('host', 'device'), default='host', help='where the light programmes run: one host controller for the whole batch '
                    '(the index tensor is copied over every step), or on the device with a clock per scene (traffic_controls.ProgrammedTrafficLightControl)')
    ap.add_argument('--stop-lines', type=int, default=0, metavar='K', help='observe the K nearest stop lines ahead (compute_stop_lines) instead of images')
    ap.add_argument('--lanes', type=int, default=0, metavar='K', help='observe the K nearest lanes as polylines (compute_lanes) instead of images')
    ap.add_argument('--npcs', type=int, default=0, metavar='N', help='N lane-following NPCs per scene (behavior.LaneFollowingNPCController)')
    ap.add_argument('--give-way', action='store_true', help='the NPCs give way to each other at junctions (LaneFollowingNPCController(give_way=True))')
    ap.add_argument('--route', type=float, default=0.0, metavar='METRES', help='deal every agent a route of METRES on the lane graph (goals.RouteGoal)')
    ap.add_argument('--route-to', action='store_true', help='deal every agent the shortest route to a random on-lane destination (goals.RouteGoal.to)')
    ap.add_argument('--route-grad', action='store_true', help='descend a route loss (advance, lateral, heading) to the actions through the simulator')
    ap.add_argument('--ttc-grad', action='store_true', help='one step: differentiate a time-to-collision penalty (within --ttc seconds, default 5) to the '
                    'actions through the simulator (compute_time_to_collision(differentiable=True))')
    ap.add_argument('--neighbors-grad', action='store_true', help='one step: differentiate a keep-your-distance penalty on the features of the --neighbors K '
                    '(default 8) nearest agents to the actions through the simulator (compute_neighbors(differentiable=True))')
    ap.add_argument('--scan-grad', action='store_true', help='one step: differentiate a keep-clear-of-the-road-edge penalty on the road ranges of the --scan '
                    'RAYS (default 64) rays to the actions through the simulator (compute_range_scan(differentiable=True))')
    ap.add_argument('--lanes-grad', action='store_true', help='one step: differentiate a lane-keeping penalty on lateral and sin_rel of the nearest of the '
                    '--lanes K (default 6) lanes to the actions through the simulator (compute_lanes(differentiable=True))')
    ap.add_argument('--stop-lines-grad', action='store_true', help='one step: differentiate a do-not-cross-the-red-line penalty on x and distance of the '
                    'nearest of the --stop-lines K (default 4) lines to the actions through the simulator (compute_stop_lines(differentiable=True))')
    ap.add_argument('--wrong-way-grad', action='store_true', help='one step: differentiate the wrong-way loss to the actions through the simulator '
                    '(compute_wrong_way(differentiable=True)): it reaches them through psi alone')
    args = ap.parse_args()
    if (args.scan > 0) + (args.neighbors > 0) + (args.stop_lines > 0) + (args.lanes > 0) > 1:
        ap.error('--scan, --neighbors, --stop-lines and --lanes are observations in place of the image: choose one')
    if args.give_way and not args.npcs:
        ap.error('--give-way is an option of the NPCs: give --npcs N too')
    if args.route and args.route_to:
        ap.error('--route and --route-to are two ways to deal the one route an agent has')
    dev = torch.device('cuda', 0)
    gold = os.path.join(ROOT, 'tests', 'golden')
    lanes = lanelet2.load_lanelet_map(os.path.join(gold, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    cfg = load_map_config(os.path.join(gold, 'maps', 'carla_Town01', 'metadata.json'))
    sim, _, _ = bench.build_simulator(args.batch, args.agents, dev, seed=0, lanelet_map=lanes)
    # traffic lights: by default the programmes run on the host, the device sees one index per light and step
    controls = {k: v.extend(args.batch).to(dev) for k, v in traffic_controls_from_map_config(cfg).items()}
    if args.lights == 'device':
        # ... with --lights device they run on the device: sim.step ticks every scene's own clocks in one launch, and a scene's lights are reset with
        # the scene, from (seed, scene id) like its spawn -- here once, for the episodes the batch starts with
        episode_ids = torch.arange(args.batch, device=dev)
        controls['traffic_light'] = programmed_traffic_lights_from_map_config(cfg, args.batch, dev, dt=0.1, seed=0)
        controls['traffic_light'].reset(scene_ids=episode_ids)
    sim.traffic_controls = controls
    if args.npcs:
        # NPC traffic: placed on the lanes clear of the agents (one launch), then on rails along the lane graph, one launch per step.  They drive on
        # revert_map of the town: the file stores its lanelets against the direction of travel, and the package's stop lines lie at the END of the
        # reverted lanelets -- ahead of an NPC that approaches a junction, where a red light has to stop it.
        from torchdrivesim_amd.behavior import LaneFollowingNPCController, heuristic_initialize_batch
        npc_lanes = lanelet2.revert_map(lanes)
        agents = torch.cat([sim.get_state()[..., :2], sim.get_agent_size(), sim.get_state()[..., 2:3]], dim=-1)
        attributes, npc_state, placed = heuristic_initialize_batch(npc_lanes, args.batch, args.npcs, seed=1, occupied=agents, on_failure='mask', device=dev)
        sim.npc_controller = LaneFollowingNPCController(npc_lanes, attributes[..., :2].contiguous(), npc_state, placed, seed=1, give_way=args.give_way)
    if args.route:
        # route goals: every agent is snapped to the lane under it and dealt a route from there (two launches); then one launch per step.  On
        # revert_map of the town, like the NPCs: the file stores its lanelets against the direction of travel.
        from torchdrivesim_amd.goals import RouteGoal
        sim.route_goals = RouteGoal.sample(lanelet2.revert_map(lanes), sim.get_state(), sim.get_present_mask(), seed=2, length=args.route)
    if args.route_to:
        # routes to a destination: the destinations are the poses of a second on-lane initialisation; agents and destinations are snapped to their
        # lanes and every agent is dealt the shortest route between the two (the first call builds the map's distance table, once)
        from torchdrivesim_amd.behavior import heuristic_initialize_batch
        from torchdrivesim_amd.goals import RouteGoal
        route_lanes = lanelet2.revert_map(lanes)
        _, destination, found = heuristic_initialize_batch(route_lanes, args.batch, args.agents, seed=3, on_failure='mask', device=dev)
        sim.route_goals = RouteGoal.to(route_lanes, sim.get_state(), destination[..., :3].contiguous(), present_mask=sim.get_present_mask() & found)
    if args.route_grad:
        return route_grad_loop(args, sim, lanes, dev)
    if args.ttc_grad:
        return ttc_grad_step(args, sim, dev)
    if args.neighbors_grad:
        return neighbors_grad_step(args, sim, dev)
    if args.lanes_grad:
        return lanes_grad_step(args, sim, dev)
    if args.scan_grad:
        return scan_grad_step(args, sim, dev)
    if args.stop_lines_grad:
        return stop_lines_grad_step(args, sim, dev)
    if args.wrong_way_grad:
        return wrong_way_grad_step(args, sim, dev)
    routed = bool(args.route) or args.route_to
    replanned = torch.zeros((), device=dev)
    programme = cfg.traffic_light_controller
    light_ids = [s.actor_id for s in cfg.stoplines if s.agent_type == 'traffic_light']
    res = Resolution(args.res, args.res)
    g = torch.Generator(device=dev).manual_seed(0)
    totals = {k: torch.zeros((), device=dev) for k in ('collision', 'offroad', 'wrong_way', 'red_light')}     # summed on the device: no sync per step
    advanced = torch.zeros((), device=dev)
    ttc_sums = torch.zeros(3, device=dev)           # agents with a time to collision below 2 s (as a share, per step), the finite times, how many
    warmup = 3                                   # the first steps build the device maps, lane tables and workspaces (once per simulator): not timed
    for it in range(warmup + args.steps):
        if it == warmup:
            for v in totals.values():
                v.zero_()
            advanced.zero_()
            ttc_sums.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        action = torch.rand((args.batch, args.agents, 2), device=dev, generator=g) * 2 - 1
        if args.lights == 'host':
            programme.tick(0.1)
            controls['traffic_light'].set_state(current_light_state_tensor_from_controller(programme, light_ids).unsqueeze(0).expand(args.batch, -1).to(dev))
        sim.step(action)
        if args.scan:
            scan = sim.compute_range_scan(n_rays=args.scan, max_range=args.scan_range)
            obs = torch.stack([scan.agents, scan.road], dim=-1) / args.scan_range        # (B, A, R, 2) in [0, 1]: distance to the nearest other agent, to the road edge
        elif args.neighbors:
            near = sim.compute_neighbors(k=args.neighbors, max_distance=args.scan_range)
            obs = near.features                                              # (B, A, K, 8): Neighbors.FEATURES per slot, zeros where near.mask is False
        elif args.stop_lines:
            lines = sim.compute_stop_lines(k=args.stop_lines, max_distance=args.scan_range)
            colour = torch.nn.functional.one_hot((lines.state + 1).long(), 4)[..., 1:]                  # red / yellow / green, all 0 in an empty slot
            obs = torch.cat([lines.features, colour.to(lines.features.dtype)], dim=-1)                 # (B, A, K, 11): StopLines.FEATURES + the colour
        elif args.lanes:
            # the map of a vector policy: per slot Lanes.FEATURES and 8 points 4 m apart that follow the lane graph while the way is unambiguous.
            # Directions are those of the simulator's lanelet map, which this package stores against the direction of travel (see --npcs): the
            # agent's own lane reads cos < 0 here; Simulator(lanelet_map=revert_map(...)) gives the other reading.
            near_lanes = sim.compute_lanes(k=args.lanes, max_distance=args.scan_range)
            obs = torch.cat([near_lanes.features, near_lanes.points.flatten(-2)], dim=-1)             # (B, A, K, 8 + 16), zeros where near_lanes.mask is False
        else:
            obs = sim.render_egocentric(res=res, fov=35.0)                   # (B, A, 3, H, W): what a policy would consume
        if routed:
            route = sim.compute_route_progress()                           # what sim.step has just computed: the dense term of a reward ...
            advanced += route.advance.sum()
            goal_obs = route.lookahead / (args.route or 64.0)               # ... and (B, A, 16, 2): where the route goes, in the agent's frame
        if args.route_to:
            # plan again, on the device and without a synchronisation, for the agents that have left their route and for those at the end of a
            # route that was cut at 16 lanelets; everybody else keeps route and progress
            again = route.off_route | (sim.route_goals.completed & sim.route_goals.truncated)
            replanned += again.sum()
            sim.route_goals.resample_to(sim.get_state(), mask=again, present_mask=sim.get_present_mask())
        if args.ttc:
            # where compute_collision says that it has happened, this says that it is about to: +inf for an agent with nothing on its course
            first = sim.compute_time_to_collision(k=1, horizon=args.ttc).min                          # (B, A) seconds
            finite = torch.isfinite(first)
            ttc_sums += torch.stack([(first < 2.0).float().mean(), torch.where(finite, first, torch.zeros_like(first)).sum(), finite.float().sum()])
        totals['collision'] += (sim.compute_collision() > 0).float().mean()
        totals['offroad'] += (sim.compute_offroad() > 0).float().mean()
        totals['wrong_way'] += (sim.compute_wrong_way() > 0).float().mean()
        totals['red_light'] += sim.compute_traffic_lights_violations().float().mean()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f'{args.steps} steps of {args.batch} x {args.agents} agents, observations {tuple(obs.shape)}: {1e3 * dt / args.steps:.2f} ms per step, '
          f'{args.batch * args.agents * args.steps / dt / 1e6:.2f} M agent-steps/s')
    if args.neighbors:
        print(f'{args.neighbors} neighbour slots within {args.scan_range:g} m: {float(near.mask.float().mean()):.3f} filled, nearest at '
              f'{float(near.features[..., :2].norm(dim=-1)[near.mask[..., 0], 0].mean()):.1f} m on average')
    if args.stop_lines:
        red = (lines.state == 0) & lines.mask
        print(f'{args.stop_lines} stop-line slots within {args.scan_range:g} m ahead: {float(lines.mask.float().mean()):.3f} filled, {float(red.float().mean()):.3f} '
              f'red; the nearest changes in {float(lines.features[..., 0, 6][lines.mask[..., 0]].mean()):.1f} s on average')
    if args.lanes:
        print(f'{args.lanes} lane slots within {args.scan_range:g} m: {float(near_lanes.mask.float().mean()):.3f} filled, '
              f'{float(near_lanes.n_valid[near_lanes.mask].float().mean()):.2f} of {near_lanes.points.shape[-2]} polyline points valid on average')
    if args.ttc:
        below, total, count = ttc_sums.tolist()
        print(f'time to collision within {args.ttc:g} s: {below / args.steps:.3f} of the agents per step below 2 s, '
              f'{count / (args.steps * args.batch * args.agents):.3f} with one at all, ' + (f'{total / count:.2f} s on average' if count else 'none to average'))
    if args.npcs:
        c = sim.npc_controller
        print(f'{args.npcs} NPCs per scene: {float((c.lane >= 0).float().mean()):.3f} on a lane, mean speed {float(c.npc_state[..., 3].mean()):.2f} m/s, '
              f'{float((c.leader != -1).float().mean()):.3f} behind a leader or a red light, {int(c.hops.sum())} lanelet changes' +
              (f', {float((c.yield_to >= 0).float().mean()):.3f} giving way at a junction' if args.give_way else ''))
    if args.route:
        r = sim.route_goals
        print(f'routes of {args.route:g} m: {float(r.valid.float().mean()):.3f} of the agents have one (mean {float(r.length.sum() / r.valid.sum().clamp(min=1)):.1f} m over '
              f'{float(r.n.sum() / r.valid.sum().clamp(min=1)):.1f} lanelets), lookahead {tuple(goal_obs.shape)}; advanced {float(advanced) / max(1, int(r.valid.sum())):.2f} m '
              f'per agent in {args.steps} steps, {float(r.completed.float().mean()):.3f} arrived, {float(route.off_route.float().mean()):.3f} off their route now')
    if args.route_to:
        r = sim.route_goals
        print(f'routes to a destination: {float(r.valid.float().mean()):.3f} of the agents have one (mean {float(r.length.sum() / r.valid.sum().clamp(min=1)):.1f} m over '
              f'{float(r.n.sum() / r.valid.sum().clamp(min=1)):.1f} lanelets, {float(r.truncated.float().mean()):.3f} cut at 16 lanelets), lookahead '
              f'{tuple(goal_obs.shape)}; advanced {float(advanced) / max(1, int(r.valid.sum())):.2f} m per agent in {args.steps} steps, {int(replanned)} routes '
              f'planned again, {float(r.completed.float().mean()):.3f} arrived')
    print('fraction of agents per step: ' + ', '.join(f'{k} {float(v) / args.steps:.3f}' for k, v in totals.items()))


if __name__ == '__main__':
    main()
