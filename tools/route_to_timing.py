"""Launch times of routes to a destination (goals.RouteGoal.to / resample_to, csrc/route_to.hip) on one MI355X, and in the SAME run what they are
to be weighed against: RouteGoal.resample, which does the same walk with a Philox draw in place of up to two table reads per hop.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch; the destinations are the poses of a second on-lane
initialisation (another seed).  One child process under `timeout` measures, in this order:
    table_build     tds_lane_distances_f64 on the town's lane table (124 x 124), each call into a new tensor: the one-off cost of the first
                    RouteGoal.to with a map (the allocation of the tensor included)
    resample        RouteGoal.resample of routes of --length metres: torch.sin / cos, one lane_snap_kernel and one route_sample_kernel launch
    resample_to     RouteGoal.resample_to to the stored destinations: torch.sin / cos, one lane_snap_kernel and one route_to_kernel launch
    snap_only       the part the two share: the copy of the poses, torch.sin / cos and the lane_snap_kernel launch
Each: --warmup calls, then HIP events around each of --reps calls; min / median / max.  resample and resample_to alternate call by call, so
neither sees a warmer device than the other.  One run on one device: the figures say what this run measured, not what every run will.

    python tools/route_to_timing.py [--batch 1024] [--agents 64] [--length 200] [--reps 20] [--warmup 3] [--out profiles/route_to_timing.json]
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
TIMEOUT_S = 400


def timed(fns, reps, warmup):
    """name -> sorted milliseconds; the functions take turns within every repeat"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for r in range(reps):
        for k, fn in fns.items():
            ev[k][r][0].record()
            fn()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: sorted(a.elapsed_time(b) for a, b in ev[k]) for k in fns}


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import lane_follow_timing
    from torchdrivesim_amd import _native as nat, _ops
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    from torchdrivesim_amd.goals import RouteGoal
    from torchdrivesim_amd.infractions import LANELET_TAGS_TO_EXCLUDE
    dev = torch.device('cuda', 0)
    B, A = args.batch, args.agents
    sim = lane_follow_timing.build(B, A, 0, dev, follow=False)
    lanes = sim.lanelet_map[0]
    state, present = sim.get_state(), sim.get_present_mask()
    _, destination, found = heuristic_initialize_batch(lanes, B, A, seed=7, device=dev)
    table = lanes.table(dev, LANELET_TAGS_TO_EXCLUDE)

    def build_table():                                                       # what _ops.lane_distances does the first time, into a tensor of its own
        to_go = torch.empty((table.n_lanelets, table.n_lanelets), dtype=torch.float64, device=dev)
        nat.call('tds_lane_distances_f64', dev, table.handle, to_go)
        return to_go

    rows = [dict(step='table_build', lanelets=table.n_lanelets, table_bytes=8 * table.n_lanelets ** 2, ms=timed(dict(t=build_table), args.reps, args.warmup)['t'])]
    sampled = RouteGoal.sample(lanes, state, present, seed=2, length=args.length)
    to = RouteGoal.to(lanes, state, destination[..., :3].contiguous(), present_mask=present & found)
    t = to._t

    def snap_only():
        t['snap_xy'].copy_(state[..., :2])
        _ops.lane_snap(to._lane_table_set(), t['snap_xy'], to._heading(state), to.tolerance, out=(t['snap_lane'], t['snap_arc'], t['snap_lateral']))

    ms = timed(dict(resample=lambda: sampled.resample(state, present_mask=present), resample_to=lambda: to.resample_to(state, present_mask=present & found),
                    snap_only=snap_only), args.reps, args.warmup)
    valid = to.valid
    rows.append(dict(step='resample', rows=B * A, ms=ms['resample'], rows_with_a_route=round(float(sampled.valid.float().mean()), 4),
                     mean_lanelets=round(float(sampled.n.float().mean()), 3), mean_length=round(float(sampled.length.mean()), 2)))
    rows.append(dict(step='resample_to', rows=B * A, ms=ms['resample_to'], rows_with_a_route=round(float(valid.float().mean()), 4),
                     mean_lanelets=round(float(to.n.float().mean()), 3), mean_length=round(float(to.length.mean()), 2),
                     truncated=round(float(to.truncated.float().mean()), 4), mean_rest_of_truncated=round(float(to.rest[to.truncated].mean()), 2)))
    rows.append(dict(step='snap_only', rows=B * A, ms=ms['snap_only']))
    for r in rows:
        m = r.pop('ms')
        r.update(reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4))
    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip, rows=rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--length', type=float, default=200.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'route_to_timing.json'))
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents),
           '--length', str(args.length), '--reps', str(args.reps), '--warmup', str(args.warmup)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got['rows']}
    ratio = by['resample_to']['ms_median'] / by['resample']['ms_median']
    doc = dict(date=datetime.date.today().isoformat(), device=got['device'], torch=got['torch'], hip=got['hip'], map='carla_Town01', batch=args.batch,
               agents=args.agents, route_length=args.length,
               what='HIP events around each call after warm-up, all in one process; resample, resample_to and snap_only take turns within every repeat',
               resample_to_over_resample=round(ratio, 3), expectation_within_2x_resample_met=ratio <= 2.0, rows=got['rows'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: by[k]['ms_median'] for k in by}))


if __name__ == '__main__':
    main()
