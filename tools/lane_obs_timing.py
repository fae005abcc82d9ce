"""Times of the lane observations (Simulator.compute_lanes; csrc/lane_obs.hip, K8) on one MI355X, and in the SAME run what they are to be weighed
against:

    lanes        Simulator.compute_lanes()                  the defaults: k = 6, 8 points 4 m apart, 30 m
    snap         lanelet2.snap_to_lanes of the same poses   the closest relative: one foot search, in one grid cell
    neighbors    Simulator.compute_neighbors(k=8)
    stop_lines   Simulator.compute_stop_lines(k=4)
    image_64     Simulator.render_egocentric at 64 x 64     the cheapest image of the same scene: what an observation for a policy that does
                                                            not look at images is expected to stay below

Scene: Town01 (124 lanelets, 12 machines, 36 lights), B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch.  One child
process under `timeout` measures: --warmup calls of each, then HIP events around each of --reps calls -- the events are on the stream, so the
host's own work between them counts --, all taking turns within every repeat; min / median / max.  One run on one device: the figures say what
this run measured, not what every run will.

    python tools/lane_obs_timing.py [--batch 1024] [--agents 64] [--reps 20] [--warmup 3] [--out profiles/lane_obs_timing.json] [--trace-dir DIR]

--trace-dir: afterwards compute_lanes and snap_to_lanes alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters);
the kernel statistics are kept as DIR/lane_obs_kernel_stats.csv and the rows of the two kernels go into the JSON: the time per dispatch.
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
PACKAGE = os.path.join(ROOT, 'tests', 'golden', 'maps', 'carla_Town01', 'metadata.json')
KERNELS = ('lane_obs_kernel', 'lane_snap_kernel')


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import range_scan_timing
    from route_to_timing import timed
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.map import load_map_config, programmed_traffic_lights_from_map_config
    from torchdrivesim_amd.utils import Resolution
    dev = torch.device('cuda', 0)
    B, A = args.batch, args.agents
    sim = range_scan_timing.build(B, A, dev)
    lanes = lanelet2.load_lanelet_map(range_scan_timing.OSM, origin=(0.0, 0.0))
    sim.lanelet_map = [lanes] * B
    state = sim.get_state()
    fns = dict(lanes=lambda: sim.compute_lanes(), snap=lambda: lanelet2.snap_to_lanes(lanes, state))
    if not args.only_lanes:
        sim.traffic_controls = {'traffic_light': programmed_traffic_lights_from_map_config(load_map_config(PACKAGE), B, dev, dt=0.1, seed=0)}
        res = Resolution(64, 64)
        fns.update(neighbors=lambda: sim.compute_neighbors(k=8), stop_lines=lambda: sim.compute_stop_lines(k=4),
                   image_64=lambda: sim.render_egocentric(res=res))
    ms = timed(fns, args.reps, args.warmup)
    obs = sim.compute_lanes()
    rows = []
    for step, m in ms.items():
        rows.append(dict(step=step, reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4)))
        if step == 'lanes':
            filled = obs.mask
            rows[-1].update(bytes=sum(t.numel() * 4 for t in (obs.features, obs.points, obs.n_valid, obs.index)), filled_slots=round(float(filled.float().mean()), 4),
                            mean_n_valid=round(float(obs.n_valid[filled].float().mean()), 4))
    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip, lanelets=len(lanes.laneletLayer),
                          rows=rows)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--reps', str(reps or args.reps),
            '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """compute_lanes and snap_to_lanes alone under rocprofv3 --kernel-trace --stats -> the statistics of the two kernels"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'lane_obs')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'lane_obs', '--',
           *child(args, '--only-lanes', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = [r for r in rows if any(k in r['Name'] for k in KERNELS)]
    if len(mine) != len(KERNELS):
        sys.exit(f'the trace under {out_dir} does not hold {KERNELS}')
    keep = os.path.join(args.trace_dir, 'lane_obs_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/lane_obs_timing.py --measure --only-lanes --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, Town01; the calls of the set-up -- map, spawn -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12] + [r for r in mine if r not in rows[:12]]:
            w.writerow({k: (v if len(v) < 160 else v[:157] + '...') for k, v in r.items()})
    return dict(stats_file=os.path.basename(keep),
                kernels=[dict(kernel=next(k for k in KERNELS if k in r['Name']), calls=int(r['Calls']), mean_ms=round(float(r['AverageNs']) / 1e6, 4),
                              min_ms=round(float(r['MinNs']) / 1e6, 4), max_ms=round(float(r['MaxNs']) / 1e6, 4)) for r in mine])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lane_obs_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace the two lane kernels with rocprofv3 and keep their statistics here')
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    ap.add_argument('--only-lanes', action='store_true', help='(internal) compute_lanes and snap_to_lanes alone')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    done = subprocess.run(['timeout', '-k', '10', str(TIMEOUT_S), *child(args)], capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got['rows']}
    med = lambda k: by[k]['ms_median']      # noqa: E731
    doc = dict(date=datetime.date.today().isoformat(), device=got['device'], torch=got['torch'], hip=got['hip'], map='carla_Town01', lanelets=got['lanelets'],
               batch=args.batch, agents=args.agents, k=6, n_points=8, spacing=4.0, max_distance=30.0,
               what='HIP events on the stream around each call after warm-up (the host\'s work between them counts), all in one process; the calls take '
                    'turns within every repeat',
               lanes_over_image_64=round(med('lanes') / med('image_64'), 5), expectation_lanes_below_the_64x64_image_met=med('lanes') < med('image_64'),
               lanes_over_snap=round(med('lanes') / med('snap'), 5), lanes_over_neighbors=round(med('lanes') / med('neighbors'), 5),
               lanes_over_stop_lines=round(med('lanes') / med('stop_lines'), 5), rows=got['rows'])

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
