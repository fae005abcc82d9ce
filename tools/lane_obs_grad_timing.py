"""Launch times of the differentiable lane observations (Simulator.compute_lanes(differentiable=True), csrc/lane_obs_bwd.hip) on one MI355X, and
in the SAME run what they are to be weighed against: today's call and K8's forward launch -- code this feature leaves as it was.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch (the scene of tools/lane_obs_timing.py).  One child
process under `timeout` measures, taking turns call by call:
    call                 compute_lanes as it always was: one lane_obs_kernel launch
    call_differentiable  the same with differentiable=True on a state that requires grad: the poses and [sin, cos] with their graph, the same launch
    forward_launch       tds_lane_observations_multi alone: the lane_obs_kernel launch
    backward_launch      tds_lane_observations_bwd_multi alone, random incoming gradients on features and points: the lane_obs_bwd_kernel launch
--warmup rounds, then HIP events around each call of --reps rounds; median (min - max).  The expectation to report against: the backward launch is
no slower than K8's forward launch of the same run, the margin being that launch's own min-max spread.  One run on one device: the figures say what
this run measured, not what every run will.

    python tools/lane_obs_grad_timing.py [--batch 1024] [--agents 64] [--k 6] [--n-points 8] [--spacing 4] [--max-distance 30] [--reps 20]
                                         [--warmup 3] [--out profiles/lane_obs_grad_timing.json] [--trace-dir DIR]

--trace-dir: afterwards the two launches alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the kernel
statistics are kept as DIR/lane_obs_grad_kernel_stats.csv and the rows of the two kernels go into the JSON: the time per dispatch.
"""
import argparse
import csv
import datetime
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
STEPS = ('call', 'call_differentiable', 'forward_launch', 'backward_launch')
TIMEOUT_S = 400
KERNELS = ('lane_obs_kernel', 'lane_obs_bwd_kernel')


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import range_scan_timing
    from route_to_timing import timed
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops, lanelet2
    dev = torch.device('cuda', 0)
    B, A, K, P = args.batch, args.agents, args.k, args.n_points
    sim = range_scan_timing.build(B, A, dev)
    lanes = lanelet2.load_lanelet_map(range_scan_timing.OSM, origin=(0.0, 0.0))
    sim.lanelet_map = [lanes] * B
    kw = dict(k=K, n_points=P, spacing=args.spacing, max_distance=args.max_distance)
    plain = sim.get_state()
    leaf = plain.detach().clone().requires_grad_(True)
    lane_set = sim._lane_tables(dev)                         # built here, before anything is timed
    xy, sc = plain.detach()[..., :2].contiguous(), _ops.heading_sc(plain.detach()[..., 2]).contiguous()
    present = _ops._u8(sim.get_present_mask())
    gen = torch.Generator(device=dev).manual_seed(0)
    features, points = torch.empty((B, A, K, 8), device=dev), torch.empty((B, A, K, P, 2), device=dev)
    n_valid, index = torch.empty((B, A, K), dtype=torch.int32, device=dev), torch.empty((B, A, K), dtype=torch.int32, device=dev)
    g_features, g_points = torch.randn((B, A, K, 8), device=dev, generator=gen), torch.randn((B, A, K, P, 2), device=dev, generator=gen)
    g_xy, g_sc = torch.empty((B, A, 2), device=dev), torch.empty((B, A, 2), device=dev)

    def call():
        sim.kinematic_model.set_state(plain)
        return sim.compute_lanes(**kw)

    def call_differentiable():
        sim.kinematic_model.set_state(leaf)
        return sim.compute_lanes(differentiable=True, **kw)

    def forward_launch():
        nat.call('tds_lane_observations_multi', dev, lane_set.handle, lane_set.scene_map, xy, sc, present, features, points, n_valid, index, B, A, K, P,
                 args.spacing, args.max_distance)

    def backward_launch():
        nat.call('tds_lane_observations_bwd_multi', dev, lane_set.handle, lane_set.scene_map, xy, sc, index, g_features, g_points, g_xy, g_sc, B, A, K, P,
                 args.spacing)

    forward_launch()                                         # the index exists before the backward is first warmed up
    fns = dict(forward_launch=forward_launch, backward_launch=backward_launch)
    if not args.only_launches:
        fns = dict(call=call, call_differentiable=call_differentiable, **fns)
    ms = timed(fns, args.reps, args.warmup)
    rows = []
    for name, m in ms.items():
        rows.append(dict(step=name, reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4)))
    forward_launch()
    backward_launch()
    torch.cuda.synchronize()
    assert bool((g_xy != 0).any()) and bool((g_sc != 0).any()) and bool((index >= 0).any()) and bool(torch.isfinite(g_xy).all())
    if not args.only_launches:
        t = call_differentiable()
        assert t.features.grad_fn is not None and torch.equal(t.features.detach(), features) and torch.equal(t.points.detach(), points) and \
            torch.equal(t.index, index)
        sim.kinematic_model.set_state(plain)
    filled = index >= 0
    print(json.dumps(dict(rows=rows, slots=int(index.numel()), slots_filled=round(float(filled.float().mean()), 4),
                          points_valid=round(float(n_valid.sum()) / (index.numel() * P), 4), mean_n_valid=round(float(n_valid[filled].float().mean()), 4),
                          observers_with_a_gradient=round(float((g_xy != 0).any(-1).float().mean()), 4), lanelets=len(lanes.laneletLayer),
                          device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--k', str(args.k),
            '--n-points', str(args.n_points), '--spacing', str(args.spacing), '--max-distance', str(args.max_distance), '--reps', str(reps or args.reps),
            '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """the two launches alone under rocprofv3 --kernel-trace --stats -> the statistics of their kernels"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'lane_obs_grad')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'lane_obs_grad', '--',
           *child(args, '--only-launches', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = {k: [r for r in rows if re.search(r'(?<![A-Za-z0-9_])' + k + r'(?![A-Za-z0-9_])', r['Name'])] for k in KERNELS}        # the whole name
    if not all(mine.values()):
        sys.exit(f'the trace under {out_dir} does not hold all of {KERNELS}')
    keep = os.path.join(args.trace_dir, 'lane_obs_grad_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/lane_obs_grad_timing.py --measure --only-launches --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, k = {args.k}, {args.n_points} points every {args.spacing} m, {args.max_distance} m; the calls of the set-up '
                f'-- map, spawn -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12] + [r for k in KERNELS for r in mine[k] if r not in rows[:12]]:
            w.writerow({k: (v if len(v) < 160 else v[:157] + '...') for k, v in r.items()})
    out = []
    for k in KERNELS:
        r = mine[k][0]
        out.append(dict(kernel=k, stats_file=os.path.basename(keep), calls=int(r['Calls']), mean_ms=round(float(r['AverageNs']) / 1e6, 4),
                        min_ms=round(float(r['MinNs']) / 1e6, 4), max_ms=round(float(r['MaxNs']) / 1e6, 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--k', type=int, default=6)
    ap.add_argument('--n-points', type=int, default=8)
    ap.add_argument('--spacing', type=float, default=4.0)
    ap.add_argument('--max-distance', type=float, default=30.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lane_obs_grad_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace the two launches with rocprofv3 and keep their kernel statistics here')
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    ap.add_argument('--only-launches', action='store_true', help='(internal) the two launches alone')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    done = subprocess.run(['timeout', '-k', '10', str(TIMEOUT_S), *child(args)], capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got.pop('rows')}
    bwd, fwd = by['backward_launch'], by['forward_launch']
    margin = round(fwd['ms_max'] - fwd['ms_min'], 4)
    doc = dict(date=datetime.date.today().isoformat(), device=got.pop('device'), torch=got.pop('torch'), hip=got.pop('hip'), map='carla_Town01', batch=args.batch,
               agents=args.agents, k=args.k, n_points=args.n_points, spacing=args.spacing, max_distance=args.max_distance,
               what='HIP events around each call after warm-up, ONE process, the four calls taking turns; `call` and `forward_launch` are the code paths of the '
                    'parent commit, measured again in this run.  Measured: the host-side launches and their kernels as the events see them.  Not measured: a '
                    'loss and autograd\'s walk to the backward node, hardware counters, any other scene, K or P',
               **got, backward_launch_over_forward_launch=round(bwd['ms_median'] / fwd['ms_median'], 3), margin_ms_forward_spread=margin,
               expectation_backward_no_slower_than_forward_met=bwd['ms_median'] <= fwd['ms_median'] + margin,
               call_differentiable_over_call=round(by['call_differentiable']['ms_median'] / by['call']['ms_median'], 3), rows=[by[k] for k in STEPS])

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')

    write()
    print(json.dumps({k: f"{by[k]['ms_median']} ({by[k]['ms_min']} - {by[k]['ms_max']})" for k in STEPS}), flush=True)
    if args.trace_dir:                                       # (the timings are on disk whatever the profiler does)
        os.makedirs(args.trace_dir, exist_ok=True)
        doc['kernel_trace'] = kernel_trace(args)
        write()
        print(json.dumps(doc['kernel_trace']), flush=True)


if __name__ == '__main__':
    main()
