"""Launch times of the differentiable route step (goals.RouteGoal(differentiable=True), csrc/route_bwd.hip) on one MI355X, and in the SAME run
what they are to be weighed against: today's step, on the code path this feature leaves as it was.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch, every agent with a route of --length metres and K
lookahead points (the scene of tools/route_goal_timing.py).  One child process under `timeout` measures, taking turns call by call:
    step                 RouteGoal.step as it always was: torch.sin / cos and one route_progress_kernel launch
    step_differentiable  RouteGoal.step with differentiable=True on a state that requires grad: torch.sin / cos (with their graph), the same launch,
                         the clone of the cursor and the six clones of the float outputs
    forward_launch       _ops.route_progress alone: the route_progress_kernel launch
    backward_launch      tds_route_progress_bwd_multi alone, all six incoming gradients given: the route_progress_bwd_kernel launch
--warmup rounds, then HIP events around each call of --reps rounds; median (min - max).  One run on one device: the figures say what this run
measured, not what every run will.  No counters are taken.

    python tools/route_grad_timing.py [--batch 1024] [--agents 64] [--length 200] [--lookahead 16] [--reps 20] [--warmup 3]
                                      [--out profiles/route_grad_timing.json]
"""
import argparse
import datetime
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
STEPS = ('step', 'step_differentiable', 'forward_launch', 'backward_launch')
TIMEOUT_S = 300


def measure(args):
    """the child process: all four, taking turns; one JSON line"""
    import torch
    import lane_follow_timing
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.goals import RouteGoal
    dev = torch.device('cuda', 0)
    B, A, K = args.batch, args.agents, args.lookahead
    sim = lane_follow_timing.build(B, A, 0, dev, follow=False)
    state, present = sim.get_state().detach().clone(), sim.get_present_mask()
    plain = RouteGoal.sample(sim.lanelet_map, state, present, seed=2, length=args.length, lookahead=K)
    diff = plain.copy()
    diff.differentiable = True
    leaf = state.clone().requires_grad_(True)
    sc = _ops.heading_sc(state[..., 2])
    g = torch.Generator(device=dev).manual_seed(0)
    grads = [torch.randn(s, device=dev, generator=g) for s in ((B, A), (B, A), (B, A), (B, A, 2), (B, A), (B, A, K, 2))]      # in the order of _ops.ROUTE_FLOATS
    g_xy, g_sc = torch.empty((B, A, 2), device=dev), torch.empty((B, A, 2), device=dev)
    lanes, t = plain._lane_table_set(), plain._t
    route = [t[name] for name, _, _ in _ops.ROUTE_TENSORS]
    scene_map = _ops._scene_map(lanes, B, 'route_grad_timing')
    u8 = _ops._u8(present)

    def backward_launch():
        nat.call('tds_route_progress_bwd_multi', dev, lanes.handle, scene_map, B, A, state, state.shape[2], sc, u8, *route, t['cursor'], *grads, K, plain.spacing,
                 g_xy, g_sc)

    calls = dict(step=lambda: plain.step(state, present), step_differentiable=lambda: diff.step(leaf, present),
                 forward_launch=lambda: _ops.route_progress(lanes, state, sc, present, t, t, plain.goal_tolerance, plain.off_route_distance, plain.spacing),
                 backward_launch=backward_launch)
    for _ in range(args.warmup):
        for name in STEPS:
            calls[name]()
    torch.cuda.synchronize()
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)] for name in STEPS}
    for r in range(args.reps):
        for name in STEPS:
            ev[name][r][0].record()
            calls[name]()
            ev[name][r][1].record()
    torch.cuda.synchronize()
    rows = []
    for name in STEPS:
        ms = sorted(a.elapsed_time(b) for a, b in ev[name])
        med = ms[len(ms) // 2]
        rows.append(dict(step=name, ms_min=round(ms[0], 4), ms_median=round(med, 4), ms_max=round(ms[-1], 4), ns_per_row=round(med * 1e6 / (B * A), 2)))
    out = diff.step(leaf, present)
    assert out.progress.grad_fn is not None and bool((g_xy != 0).any())
    print(json.dumps(dict(rows=rows, rows_per_call=B * A, rows_with_a_route=round(float(plain.valid.float().mean()), 4),
                          mean_lanelets=round(float(plain.n.float().mean()), 3), device=torch.cuda.get_device_name(dev), torch=torch.__version__,
                          hip=torch.version.hip)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--length', type=float, default=200.0)
    ap.add_argument('--lookahead', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'route_grad_timing.json'))
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents),
           '--length', str(args.length), '--lookahead', str(args.lookahead), '--reps', str(args.reps), '--warmup', str(args.warmup)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got['rows']}
    ratio = by['backward_launch']['ms_median'] / by['forward_launch']['ms_median']
    doc = dict(date=datetime.date.today().isoformat(), device=got['device'], torch=got['torch'], hip=got['hip'], map='carla_Town01', batch=args.batch,
               agents=args.agents, route_length=args.length, lookahead=args.lookahead, reps=args.reps, warmup=args.warmup,
               what='HIP events around each call after warm-up, ONE process, the four calls taking turns; `step` is the code path of the parent commit, '
                    'measured again in this run.  Measured: the host-side launches and their kernels as the events see them.  Not measured: a loss and '
                    'autograd\'s walk to the backward node, hardware counters, any other scene',
               rows_per_call=got['rows_per_call'], rows_with_a_route=got['rows_with_a_route'], mean_lanelets=got['mean_lanelets'],
               backward_launch_over_forward_launch=round(ratio, 3), expectation_backward_within_2x_forward_launch_met=ratio <= 2.0,
               step_differentiable_over_step=round(by['step_differentiable']['ms_median'] / by['step']['ms_median'], 3), rows=got['rows'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: f"{by[k]['ms_median']} ({by[k]['ms_min']} - {by[k]['ms_max']})" for k in STEPS}))


if __name__ == '__main__':
    main()
