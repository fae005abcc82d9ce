"""Launch times of time to collision (Simulator.compute_time_to_collision, csrc/ttc.hip) on one MI355X, and in the SAME run what it is to be
weighed against: compute_neighbors(k=8), the other wave-per-observer kernel over the same entities, and compute_range_scan(road=False), the
agents-only range scan, which tests 64 rays per pair where this tests four axes -- the expectation is that a call costs no more than that scan.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch.  One child process under `timeout` measures:
--warmup calls of each, then HIP events around each of --reps calls, the three taking turns within every repeat so that none sees a warmer
device than the others; min / median / max.  One run on one device: the figures say what this run measured, not what every run will.

    python tools/ttc_timing.py [--batch 1024] [--agents 64] [--k 1] [--horizon 5] [--margin 0] [--reps 20] [--warmup 3]
                               [--out profiles/ttc_timing.json] [--trace-dir DIR]

--trace-dir: afterwards compute_time_to_collision alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the
kernel statistics are kept as DIR/ttc_kernel_stats.csv and the row of time_to_collision_kernel goes into the JSON: the time per dispatch.
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
TIMEOUT_S = 400
KERNEL = 'time_to_collision_kernel'


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import range_scan_timing
    from route_to_timing import timed
    dev = torch.device('cuda', 0)
    B, A = args.batch, args.agents
    sim = range_scan_timing.build(B, A, dev)
    ttc = lambda: sim.compute_time_to_collision(k=args.k, horizon=args.horizon, margin=args.margin)
    fns = dict(ttc=ttc)
    if not args.only_ttc:
        fns.update(neighbors=lambda: sim.compute_neighbors(k=8), scan_agents_only=lambda: sim.compute_range_scan(road=False))
    ms = timed(fns, args.reps, args.warmup)
    t = ttc()
    finite = torch.isfinite(t.min)
    speed = sim.get_all_agent_state()[..., 3]
    rows = [dict(step='ttc', bytes=t.ttc.numel() * 4 + t.index.numel() * 4, agents_with_a_ttc=round(float(finite.float().mean()), 4),
                 agents_overlapping=round(float((t.min == 0).float().mean()), 4),
                 mean_finite_ttc_s=round(float(t.min[finite].mean()), 4) if bool(finite.any()) else None,
                 mean_speed_m_s=round(float(speed.mean()), 4), max_speed_m_s=round(float(speed.max()), 4))]
    if not args.only_ttc:
        nb, scan = sim.compute_neighbors(k=8), sim.compute_range_scan(road=False)
        rows.append(dict(step='neighbors', bytes=nb.features.numel() * 4 + nb.index.numel() * 4))
        rows.append(dict(step='scan_agents_only', bytes=12 * scan.hit.numel()))
    for r in rows:
        m = ms[r['step']]
        r.update(reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4))
    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip, rows=rows)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--k', str(args.k),
            '--horizon', str(args.horizon), '--margin', str(args.margin), '--reps', str(reps or args.reps), '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """compute_time_to_collision alone under rocprofv3 --kernel-trace --stats -> the statistics of its kernel"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'ttc')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'ttc', '--',
           *child(args, '--only-ttc', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = [r for r in rows if KERNEL in r['Name']]
    if not mine:
        sys.exit(f'the trace under {out_dir} holds no {KERNEL}')
    keep = os.path.join(args.trace_dir, 'ttc_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ttc_timing.py --measure --only-ttc --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, k = {args.k}, {args.horizon} s, margin {args.margin} m; the calls of the set-up -- spawn -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12]:
            w.writerow({k: (v if len(v) < 160 else v[:157] + '...') for k, v in r.items()})
    r = mine[0]
    return dict(kernel=KERNEL, stats_file=os.path.basename(keep), calls=int(r['Calls']), mean_ms=round(float(r['AverageNs']) / 1e6, 4),
                min_ms=round(float(r['MinNs']) / 1e6, 4), max_ms=round(float(r['MaxNs']) / 1e6, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--horizon', type=float, default=5.0)
    ap.add_argument('--margin', type=float, default=0.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ttc_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace compute_time_to_collision with rocprofv3 and keep its kernel statistics here')
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    ap.add_argument('--only-ttc', action='store_true', help='(internal) compute_time_to_collision alone')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    done = subprocess.run(['timeout', '-k', '10', str(TIMEOUT_S), *child(args)], capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got['rows']}
    ratio = by['ttc']['ms_median'] / by['scan_agents_only']['ms_median']
    doc = dict(date=datetime.date.today().isoformat(), device=got['device'], torch=got['torch'], hip=got['hip'], map='carla_Town01', batch=args.batch,
               agents=args.agents, k=args.k, horizon=args.horizon, margin=args.margin,
               what='HIP events around each call after warm-up, all in one process; the three take turns within every repeat',
               ttc_over_scan_agents_only=round(ratio, 5), expectation_not_slower_than_scan_agents_only_met=ratio <= 1.0, rows=got['rows'])

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')

    write()
    print(json.dumps({k: by[k]['ms_median'] for k in by}), flush=True)
    if args.trace_dir:                                       # (the timings are on disk whatever the profiler does)
        os.makedirs(args.trace_dir, exist_ok=True)
        doc['kernel_trace'] = kernel_trace(args)
        write()
        print(json.dumps(doc['kernel_trace']), flush=True)


if __name__ == '__main__':
    main()
