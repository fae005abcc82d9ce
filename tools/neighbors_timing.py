"""Launch times of the neighbour observations (Simulator.compute_neighbors, csrc/neighbors.hip) on one MI355X, and in the SAME run what they are
to be weighed against: get_all_agents_relative(), the reference's dense form (about ten torch launches, a B x A x (A - 1) x 6 tensor), and
compute_range_scan(road=False), the other observation of the agents around.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch.  One child process under `timeout` measures:
--warmup calls of each, then HIP events around each of --reps calls, the three taking turns within every repeat so that none sees a warmer
device than the others; min / median / max.  One run on one device: the figures say what this run measured, not what every run will.

    python tools/neighbors_timing.py [--batch 1024] [--agents 64] [--k 8] [--max-distance 50] [--reps 20] [--warmup 3]
                                     [--out profiles/neighbors_timing.json] [--trace-dir DIR]

--trace-dir: afterwards compute_neighbors alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the kernel
statistics are kept as DIR/neighbors_kernel_stats.csv and the row of neighbors_kernel goes into the JSON: the time per dispatch.
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


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import range_scan_timing
    from route_to_timing import timed
    dev = torch.device('cuda', 0)
    B, A = args.batch, args.agents
    sim = range_scan_timing.build(B, A, dev)
    fns = dict(neighbors=lambda: sim.compute_neighbors(k=args.k, max_distance=args.max_distance))
    if not args.only_neighbors:
        fns.update(relative=lambda: sim.get_all_agents_relative(), scan_agents_only=lambda: sim.compute_range_scan(road=False))
    ms = timed(fns, args.reps, args.warmup)
    nb = sim.compute_neighbors(k=args.k, max_distance=args.max_distance)
    rows = [dict(step='neighbors', bytes=nb.features.numel() * 4 + nb.index.numel() * 4, filled_slots=round(float(nb.mask.float().mean()), 4),
                 full_rows=round(float(nb.mask.all(-1).float().mean()), 4))]
    if not args.only_neighbors:
        rel, scan = sim.get_all_agents_relative(), sim.compute_range_scan(road=False)
        rows.append(dict(step='relative', bytes=rel.numel() * 4, shape=list(rel.shape)))
        rows.append(dict(step='scan_agents_only', bytes=12 * scan.hit.numel()))
    for r in rows:
        m = ms[r['step']]
        r.update(reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4))
    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip, rows=rows)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--k', str(args.k),
            '--max-distance', str(args.max_distance), '--reps', str(reps or args.reps), '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """compute_neighbors alone under rocprofv3 --kernel-trace --stats -> the statistics of neighbors_kernel"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'neighbors')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'neighbors', '--',
           *child(args, '--only-neighbors', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = [r for r in rows if 'neighbors_kernel' in r['Name']]
    if not mine:
        sys.exit(f'the trace under {out_dir} holds no neighbors_kernel')
    keep = os.path.join(args.trace_dir, 'neighbors_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/neighbors_timing.py --measure --only-neighbors --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, k = {args.k}, {args.max_distance} m; the calls of the set-up -- spawn -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12]:
            w.writerow({k: (v if len(v) < 160 else v[:157] + '...') for k, v in r.items()})
    r = mine[0]
    return dict(kernel='neighbors_kernel', stats_file=os.path.basename(keep), calls=int(r['Calls']), mean_ms=round(float(r['AverageNs']) / 1e6, 4),
                min_ms=round(float(r['MinNs']) / 1e6, 4), max_ms=round(float(r['MaxNs']) / 1e6, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--max-distance', type=float, default=50.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neighbors_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace compute_neighbors with rocprofv3 and keep its kernel statistics here')
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    ap.add_argument('--only-neighbors', action='store_true', help='(internal) compute_neighbors alone')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    done = subprocess.run(['timeout', '-k', '10', str(TIMEOUT_S), *child(args)], capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got['rows']}
    ratio = by['neighbors']['ms_median'] / by['relative']['ms_median']
    doc = dict(date=datetime.date.today().isoformat(), device=got['device'], torch=got['torch'], hip=got['hip'], map='carla_Town01', batch=args.batch,
               agents=args.agents, k=args.k, max_distance=args.max_distance,
               what='HIP events around each call after warm-up, all in one process; the three take turns within every repeat',
               neighbors_over_relative=round(ratio, 5), expectation_not_slower_than_relative_met=ratio <= 1.0, rows=got['rows'])

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
