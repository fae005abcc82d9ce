"""Launch times of differentiable time to collision (Simulator.compute_time_to_collision(differentiable=True), csrc/ttc_bwd.hip) on one MI355X, and
in the SAME run what they are to be weighed against: today's call and today's forward launch, code this feature leaves as it was.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch (the scene of tools/ttc_timing.py).  One child process
under `timeout` measures, taking turns call by call:
    call                 compute_time_to_collision as it always was: the cat of the boxes and one time_to_collision_kernel launch
    call_differentiable  the same with differentiable=True on a state that requires grad: the boxes and [sin, cos] with their graph, the same launch
    forward_launch       tds_time_to_collision_f32 alone: the time_to_collision_kernel launch
    backward_launch      tds_time_to_collision_bwd_f32 alone, a random incoming gradient: the time_to_collision_bwd_kernel launch
--warmup rounds, then HIP events around each call of --reps rounds; median (min - max).  The expectation to report against: the backward launch
costs no more than 2 x the forward launch of the same run.  One run on one device: the figures say what this run measured, not what every run will.

    python tools/ttc_grad_timing.py [--batch 1024] [--agents 64] [--k 1] [--horizon 5] [--margin 0] [--reps 20] [--warmup 3]
                                    [--out profiles/ttc_grad_timing.json] [--trace-dir DIR]

--trace-dir: afterwards the two launches alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the kernel
statistics are kept as DIR/ttc_grad_kernel_stats.csv and the rows of the two kernels go into the JSON: the time per dispatch.
"""
import argparse
import csv
import datetime
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
STEPS = ('call', 'call_differentiable', 'forward_launch', 'backward_launch')
TIMEOUT_S = 400
KERNELS = ('time_to_collision_kernel', 'time_to_collision_bwd_kernel')


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
    kw = dict(k=K, horizon=args.horizon, margin=args.margin)
    plain = sim.get_state()
    leaf = plain.detach().clone().requires_grad_(True)
    st = plain.detach()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1).contiguous()
    sc, speed, present = _ops.heading_sc(st[..., 2]).contiguous(), st[..., 3].contiguous(), _ops._u8(sim.get_all_agent_present_mask())
    E = boxes.shape[1]
    ttc, index = torch.empty((B, A, K), device=dev), torch.empty((B, A, K), dtype=torch.int32, device=dev)
    g = torch.randn((B, A, K), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    g_boxes, g_sc, g_speed = torch.empty((B, E, 5), device=dev), torch.empty((B, E, 2), device=dev), torch.empty((B, E), device=dev)

    def call():
        sim.kinematic_model.set_state(plain)
        return sim.compute_time_to_collision(**kw)

    def call_differentiable():
        sim.kinematic_model.set_state(leaf)
        return sim.compute_time_to_collision(differentiable=True, **kw)

    def forward_launch():
        nat.call('tds_time_to_collision_f32', dev, boxes, sc, speed, present, None, ttc, index, B, A, E, K, args.horizon, args.margin)

    def backward_launch():
        nat.call('tds_time_to_collision_bwd_f32', dev, boxes, sc, speed, index, g, g_boxes, g_sc, g_speed, B, A, E, K, args.margin)

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
    contributing = (index >= 0) & (ttc > 0)
    assert bool((g_boxes != 0).any()) and bool(contributing.any())
    if not args.only_launches:
        t = call_differentiable()
        assert t.ttc.grad_fn is not None and torch.equal(t.ttc.detach(), ttc) and torch.equal(t.index, index)
        sim.kinematic_model.set_state(plain)
    print(json.dumps(dict(rows=rows, slots=int(index.numel()), slots_filled=round(float((index >= 0).float().mean()), 4),
                          slots_contributing=round(float(contributing.float().mean()), 4),
                          entities_with_a_gradient=round(float((g_boxes[..., :4] != 0).any(-1).float().mean()), 4), device=torch.cuda.get_device_name(dev),
                          torch=torch.__version__, hip=torch.version.hip)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--k', str(args.k),
            '--horizon', str(args.horizon), '--margin', str(args.margin), '--reps', str(reps or args.reps), '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """the two launches alone under rocprofv3 --kernel-trace --stats -> the statistics of their kernels"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'ttc_grad')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'ttc_grad', '--',
           *child(args, '--only-launches', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = {k: [r for r in rows if k in r['Name']] for k in KERNELS}           # (neither name is part of the other)
    if not all(mine.values()):
        sys.exit(f'the trace under {out_dir} does not hold both of {KERNELS}')
    keep = os.path.join(args.trace_dir, 'ttc_grad_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ttc_grad_timing.py --measure --only-launches --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, k = {args.k}, {args.horizon} s, margin {args.margin} m; the calls of the set-up -- spawn -- included)\n')
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
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--horizon', type=float, default=5.0)
    ap.add_argument('--margin', type=float, default=0.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ttc_grad_timing.json'))
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
    ratio = by['backward_launch']['ms_median'] / by['forward_launch']['ms_median']
    doc = dict(date=datetime.date.today().isoformat(), device=got.pop('device'), torch=got.pop('torch'), hip=got.pop('hip'), map='carla_Town01', batch=args.batch,
               agents=args.agents, k=args.k, horizon=args.horizon, margin=args.margin,
               what='HIP events around each call after warm-up, ONE process, the four calls taking turns; `call` and `forward_launch` are the code paths of the '
                    'parent commit, measured again in this run.  Measured: the host-side launches and their kernels as the events see them.  Not measured: '
                    'a loss and autograd\'s walk to the backward node, hardware counters, any other scene, K or entity count',
               **got, backward_launch_over_forward_launch=round(ratio, 3), expectation_backward_within_2x_forward_launch_met=ratio <= 2.0,
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
