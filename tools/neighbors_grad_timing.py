"""Launch times of the differentiable neighbour observations (Simulator.compute_neighbors(differentiable=True), csrc/neighbors_bwd.hip) on one
MI355X, and in the SAME run what they are to be weighed against: today's call, today's forward launch and the backward launch of time to collision
at the same B, A, E and K -- code this feature leaves as it was.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch (the scene of tools/ttc_timing.py).  One child process
under `timeout` measures, taking turns call by call:
    call                 compute_neighbors as it always was: the cat of the boxes and one neighbors_kernel launch
    call_differentiable  the same with differentiable=True on a state that requires grad: the boxes and [sin, cos] with their graph, the same launch
    forward_launch       tds_neighbors_f32 alone: the neighbors_kernel launch
    backward_launch      tds_neighbors_bwd_f32 alone, a random incoming gradient: the neighbors_bwd_kernel launch
    ttc_backward_launch  tds_time_to_collision_bwd_f32 alone on the index of its own forward (same K, horizon 5 s, no margin), a random gradient
--warmup rounds, then HIP events around each call of --reps rounds; median (min - max).  The expectation to report against: the backward launch is
no slower than the time-to-collision backward launch of the same run, the margin being that launch's own min-max spread.  The ratio to the forward
launch is reported without a bar.  One run on one device: the figures say what this run measured, not what every run will.

    python tools/neighbors_grad_timing.py [--batch 1024] [--agents 64] [--k 8] [--max-distance 50] [--reps 20] [--warmup 3]
                                          [--out profiles/neighbors_grad_timing.json] [--trace-dir DIR]

--trace-dir: afterwards the three launches alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the kernel
statistics are kept as DIR/neighbors_grad_kernel_stats.csv and the rows of the three kernels go into the JSON: the time per dispatch.
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
STEPS = ('call', 'call_differentiable', 'forward_launch', 'backward_launch', 'ttc_backward_launch')
LAUNCHES = STEPS[2:]
TIMEOUT_S = 400
KERNELS = ('neighbors_kernel', 'neighbors_bwd_kernel', 'time_to_collision_bwd_kernel')
TTC_HORIZON = 5.0


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import range_scan_timing
    from route_to_timing import timed
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    dev = torch.device('cuda', 0)
    B, A, K = args.batch, args.agents, args.k
    sim = range_scan_timing.build(B, A, dev)
    kw = dict(k=K, max_distance=args.max_distance)
    plain = sim.get_state()
    leaf = plain.detach().clone().requires_grad_(True)
    st = plain.detach()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1).contiguous()
    sc, speed, present = _ops.heading_sc(st[..., 2]).contiguous(), st[..., 3].contiguous(), _ops._u8(sim.get_all_agent_present_mask())
    E = boxes.shape[1]
    gen = torch.Generator(device=dev).manual_seed(0)
    features, index = torch.empty((B, A, K, 8), device=dev), torch.empty((B, A, K), dtype=torch.int32, device=dev)
    g = torch.randn((B, A, K, 8), device=dev, generator=gen)
    g_boxes, g_sc, g_speed = torch.empty((B, E, 5), device=dev), torch.empty((B, E, 2), device=dev), torch.empty((B, E), device=dev)
    ttc, ttc_index = torch.empty((B, A, K), device=dev), torch.empty((B, A, K), dtype=torch.int32, device=dev)
    g_ttc = torch.randn((B, A, K), device=dev, generator=gen)
    t_boxes, t_sc, t_speed = torch.empty((B, E, 5), device=dev), torch.empty((B, E, 2), device=dev), torch.empty((B, E), device=dev)
    nat.call('tds_time_to_collision_f32', dev, boxes, sc, speed, present, None, ttc, ttc_index, B, A, E, K, TTC_HORIZON, 0.0)

    def call():
        sim.kinematic_model.set_state(plain)
        return sim.compute_neighbors(**kw)

    def call_differentiable():
        sim.kinematic_model.set_state(leaf)
        return sim.compute_neighbors(differentiable=True, **kw)

    def forward_launch():
        nat.call('tds_neighbors_f32', dev, boxes, sc, speed, present, None, features, index, B, A, E, K, args.max_distance)

    def backward_launch():
        nat.call('tds_neighbors_bwd_f32', dev, boxes, sc, speed, index, g, g_boxes, g_sc, g_speed, B, A, E, K)

    def ttc_backward_launch():
        nat.call('tds_time_to_collision_bwd_f32', dev, boxes, sc, speed, ttc_index, g_ttc, t_boxes, t_sc, t_speed, B, A, E, K, 0.0)

    forward_launch()                                         # the index exists before the backward is first warmed up
    fns = dict(forward_launch=forward_launch, backward_launch=backward_launch, ttc_backward_launch=ttc_backward_launch)
    if not args.only_launches:
        fns = dict(call=call, call_differentiable=call_differentiable, **fns)
    ms = timed(fns, args.reps, args.warmup)
    rows = []
    for name, m in ms.items():
        rows.append(dict(step=name, reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4)))
    forward_launch()
    backward_launch()
    ttc_backward_launch()
    torch.cuda.synchronize()
    assert bool((g_boxes != 0).any()) and bool((index >= 0).any()) and bool((t_boxes != 0).any())
    if not args.only_launches:
        t = call_differentiable()
        assert t.features.grad_fn is not None and torch.equal(t.features.detach(), features) and torch.equal(t.index, index)
        sim.kinematic_model.set_state(plain)
    print(json.dumps(dict(rows=rows, slots=int(index.numel()), slots_filled=round(float((index >= 0).float().mean()), 4),
                          ttc_slots_filled=round(float((ttc_index >= 0).float().mean()), 4),
                          ttc_slots_contributing=round(float(((ttc_index >= 0) & (ttc > 0)).float().mean()), 4),
                          entities_with_a_gradient=round(float((g_boxes[..., :4] != 0).any(-1).float().mean()), 4), device=torch.cuda.get_device_name(dev),
                          torch=torch.__version__, hip=torch.version.hip)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--k', str(args.k),
            '--max-distance', str(args.max_distance), '--reps', str(reps or args.reps), '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """the three launches alone under rocprofv3 --kernel-trace --stats -> the statistics of their kernels"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'neighbors_grad')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'neighbors_grad', '--',
           *child(args, '--only-launches', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = {k: [r for r in rows if re.search(r'(?<![A-Za-z0-9_])' + k + r'(?![A-Za-z0-9_])', r['Name'])] for k in KERNELS}        # the whole name
    if not all(mine.values()):
        sys.exit(f'the trace under {out_dir} does not hold all of {KERNELS}')
    keep = os.path.join(args.trace_dir, 'neighbors_grad_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/neighbors_grad_timing.py --measure --only-launches --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, k = {args.k}, {args.max_distance} m; the calls of the set-up -- spawn -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12]:
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
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--max-distance', type=float, default=50.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neighbors_grad_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace the three launches with rocprofv3 and keep their kernel statistics here')
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    ap.add_argument('--only-launches', action='store_true', help='(internal) the three launches alone')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    done = subprocess.run(['timeout', '-k', '10', str(TIMEOUT_S), *child(args)], capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got.pop('rows')}
    bwd, ttc_bwd, fwd = by['backward_launch'], by['ttc_backward_launch'], by['forward_launch']
    margin = round(ttc_bwd['ms_max'] - ttc_bwd['ms_min'], 4)
    doc = dict(date=datetime.date.today().isoformat(), device=got.pop('device'), torch=got.pop('torch'), hip=got.pop('hip'), map='carla_Town01', batch=args.batch,
               agents=args.agents, k=args.k, max_distance=args.max_distance, ttc_horizon=TTC_HORIZON,
               what='HIP events around each call after warm-up, ONE process, the five calls taking turns; `call`, `forward_launch` and `ttc_backward_launch` '
                    'are the code paths of the parent commit, measured again in this run.  Measured: the host-side launches and their kernels as the events '
                    'see them.  Not measured: a loss and autograd\'s walk to the backward node, hardware counters, any other scene, K or entity count',
               **got, backward_launch_over_ttc_backward_launch=round(bwd['ms_median'] / ttc_bwd['ms_median'], 3), margin_ms_ttc_backward_spread=margin,
               expectation_backward_no_slower_than_ttc_backward_met=bwd['ms_median'] <= ttc_bwd['ms_median'] + margin,
               backward_launch_over_forward_launch=round(bwd['ms_median'] / fwd['ms_median'], 3),
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
