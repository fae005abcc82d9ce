"""Launch times of route goals (goals.RouteGoal, csrc/route.hip) on one MI355X, and in the SAME run what they are to be weighed against.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch, every agent with a route of --length metres and K
lookahead points.  Steps, each in a child process of its own under `timeout` (the first that fails ends the run; nothing more is started on the
device):
    route_sample        RouteGoal.resample: torch.sin / cos, one lane_snap_kernel and one route_sample_kernel launch
    route_step          RouteGoal.step: torch.sin / cos and one route_progress_kernel launch
    step_with_routes    a whole Simulator.step (random actions) with route_goals
    step_plain          the same Simulator.step without them
    render_64           render_egocentric of the same scene at 64 x 64
    advance_npcs        LaneFollowingNPCController.advance_npcs at B x (--npc-agents + --npcs), the scene of tools/lane_follow_timing.py
A step: --warmup calls, then HIP events around each of --reps calls; min / median / max.  One run on one device: the figures say what this run
measured, not what every run will.

    python tools/route_goal_timing.py [--batch 1024] [--agents 64] [--length 200] [--lookahead 16] [--reps 20] [--warmup 3]
                                      [--out profiles/route_goal_timing.json] [--trace-dir DIR]

--trace-dir: after the timed steps, route_step once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters), its kernel
statistics kept as DIR/route_step_kernel_stats.csv and their top rows copied into the JSON.
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
STEPS = ('route_sample', 'route_step', 'advance_npcs', 'step_with_routes', 'step_plain', 'render_64')
STEP_TIMEOUT_S = 240


def run_step(args):
    """a child process: one measurement, one JSON line"""
    import torch
    import lane_follow_timing
    from torchdrivesim_amd.goals import RouteGoal
    from torchdrivesim_amd.utils import Resolution
    dev = torch.device('cuda', 0)
    B, A = args.batch, args.agents
    extra = {}
    if args.step == 'advance_npcs':
        sim = lane_follow_timing.build(B, args.npc_agents, args.npcs, dev, follow=True)
        fn = lambda: sim.npc_controller.advance_npcs(sim)
        rows = B * args.npcs
    else:
        sim = lane_follow_timing.build(B, A, 0, dev, follow=False)
        rows = B * A
        g = torch.Generator(device=dev).manual_seed(0)
        action = torch.rand((B, A, 2), device=dev, generator=g) * 2 - 1
        goal = None
        if args.step != 'step_plain' and args.step != 'render_64':
            goal = RouteGoal.sample(sim.lanelet_map, sim.get_state(), sim.get_present_mask(), seed=2, length=args.length, lookahead=args.lookahead)
            extra = dict(rows_with_a_route=round(float(goal.valid.float().mean()), 4), mean_lanelets=round(float(goal.n.float().mean()), 3),
                         mean_length=round(float(goal.length.mean()), 2))
        if args.step == 'route_sample':
            fn = lambda: goal.resample(sim.get_state(), present_mask=sim.get_present_mask())
        elif args.step == 'route_step':
            fn = lambda: goal.step(sim.get_state(), sim.get_present_mask())
        elif args.step == 'render_64':
            fn = lambda: sim.render_egocentric(res=Resolution(64, 64), fov=35.0)
        else:
            sim.route_goals = goal
            fn = lambda: sim.step(action)
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.reps)]
    for r in range(args.reps):
        ev[2 * r].record()
        fn()
        ev[2 * r + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(args.reps))
    if args.step in ('route_step', 'step_with_routes'):
        out = goal.last_progress
        extra.update(mean_progress=round(float(out.progress.mean()), 3), off_route=round(float(out.off_route.float().mean()), 4))
    med = ms[len(ms) // 2]
    print(json.dumps(dict(step=args.step, rows=rows, reps=args.reps, warmup=args.warmup, ms_min=round(ms[0], 3), ms_median=round(med, 3), ms_max=round(ms[-1], 3),
                          ns_per_row=round(med * 1e6 / rows, 2), device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip,
                          **extra)), flush=True)


def child(args, step, reps, warmup):
    return [sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(args.batch), '--agents', str(args.agents), '--npcs', str(args.npcs),
            '--npc-agents', str(args.npc_agents), '--length', str(args.length), '--lookahead', str(args.lookahead), '--reps', str(reps), '--warmup', str(warmup)]


def kernel_trace(args, step):
    """one step under rocprofv3 --kernel-trace --stats -> the top rows of its kernel statistics"""
    import csv
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, step)
    cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'route', '--'] + \
        child(args, step, 10, 2)
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'trace of step {step} ended with status {done.returncode}: nothing more is started')
    rows, _ = trace_rows(out_dir)
    if not rows:
        sys.exit(f'trace of step {step}: rocprofv3 wrote no kernel statistics under {out_dir}')
    keep = os.path.join(args.trace_dir, f'{step}_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/route_goal_timing.py --step {step} --reps 10 --warmup 2   (B = {args.batch} x '
                f'A = {args.agents}, routes of {args.length} m, K = {args.lookahead}; the calls of the set-up -- lane tables, spawn, snap, sampling -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12]:
            w.writerow({k: (v if len(v) < 160 else v[:157] + '...') for k, v in r.items()})
    short = lambda n: n.split('(')[0][-80:] if not n.startswith('(anonymous') else n.split('::', 1)[1].split('(')[0]
    top = [dict(kernel=short(r['Name']), calls=int(r['Calls']), total_ms=round(float(r['TotalDurationNs']) / 1e6, 3), mean_ms=round(float(r['AverageNs']) / 1e6, 4),
                min_ms=round(float(r['MinNs']) / 1e6, 4), max_ms=round(float(r['MaxNs']) / 1e6, 4), percent=round(float(r['Percentage']), 2)) for r in rows[:6]]
    return dict(step=step, stats_file=os.path.basename(keep), top_kernels=top)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--npc-agents', type=int, default=32, help='exposed agents of the advance_npcs scene')
    ap.add_argument('--npcs', type=int, default=32, help='NPCs of the advance_npcs scene')
    ap.add_argument('--length', type=float, default=200.0)
    ap.add_argument('--lookahead', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'route_goal_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace route_step with rocprofv3 and keep its kernel statistics here')
    ap.add_argument('--step', choices=STEPS, help='(internal) run one measurement in this process')
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    rows, failed = [], None
    for step in STEPS:
        done = subprocess.run(['timeout', '-k', '10', str(STEP_TIMEOUT_S)] + child(args, step, args.reps, args.warmup), capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
            failed = f'step {step} ended with status {done.returncode}: nothing more was started'
            break
        rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    by = {r['step']: r for r in rows}
    if 'route_step' not in by or 'advance_npcs' not in by:
        sys.exit(failed)
    ratio = by['route_step']['ns_per_row'] / by['advance_npcs']['ns_per_row']
    doc = dict(date=datetime.date.today().isoformat(), device=rows[0]['device'], torch=rows[0]['torch'], hip=rows[0]['hip'], map='carla_Town01',
               batch=args.batch, agents=args.agents, route_length=args.length, lookahead=args.lookahead, npc_scene=[args.npc_agents, args.npcs],
               what='HIP events around each call after warm-up, one child process per step; step_plain, render_64 and advance_npcs are code this feature '
                    'does not touch, measured in the same run for comparison',
               route_step_per_row_over_advance_npcs_per_row=round(ratio, 3), expectation_at_most_2x_advance_npcs_per_row_met=ratio <= 2.0, rows=rows)
    for r in rows:
        for k in ('device', 'torch', 'hip'):
            r.pop(k)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')

    if failed:
        doc['failed'] = failed
    write()
    if failed:
        sys.exit(failed)
    if args.trace_dir:                                       # (the timings are on disk whatever the profiler does)
        os.makedirs(args.trace_dir, exist_ok=True)
        doc['kernel_trace'] = [kernel_trace(args, 'route_step')]
        print(json.dumps(doc['kernel_trace'][-1]), flush=True)
        write()
    print(json.dumps({k: by[k]['ms_median'] for k in by}))


if __name__ == '__main__':
    main()
