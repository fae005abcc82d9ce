"""Launch times of the range scan (Simulator.compute_range_scan, csrc/scan.hip) on one MI355X, and in the SAME run the observations and metrics
it stands beside: render_egocentric at 64 x 64 and 256 x 256 (float32, into a caller-owned buffer) and compute_offroad + compute_collision.

Scene: Town01, B scenes x A agents placed on the lanes by heuristic_initialize_batch, R rays, max_range metres.  Every step runs in a child process
of its own under `timeout`; the first step that fails ends the run (nothing more is started on the device).  A step: --warmup calls, then HIP
events around each of --reps calls; min / median / max.  One run on one device: the figures say what this run measured, not what every run will.

    python tools/range_scan_timing.py [--batch 1024] [--agents 64] [--rays 64] [--max-range 50] [--reps 20] [--warmup 3] [--out profiles/range_scan_timing.json]
                                      [--trace-dir DIR]

--trace-dir: after the timed steps, each of the three scan steps once more under `rocprofv3 --kernel-trace --stats` (a run of its own per step, no
counters), the kernel statistics kept as DIR/<step>_kernel_stats.csv and their top rows copied into the JSON: which kernels a call consists of and
what each of them takes.
"""
import csv
import glob
import argparse
import datetime
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OSM = os.path.join(ROOT, 'tests', 'golden', 'carla_Town01.osm.gz')
STEPS = ('scan', 'scan_road_only', 'scan_agents_only', 'render_64', 'render_256', 'offroad_collision')
STEP_TIMEOUT_S = 240


def build(B, A, dev):
    import numpy as np
    import torch
    import bench
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import CollisionMetric, Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    verts, faces, vcat, cats = bench.load_town01()
    road = BirdviewMesh(verts=torch.from_numpy(verts)[None], faces=torch.from_numpy(faces.astype(np.int64))[None], categories=cats, colors={}, zs={},
                        vert_category=torch.from_numpy(vcat.astype(np.int64))[None]).expand(B).to(dev)
    attributes, states, placed = heuristic_initialize_batch(lanelet2.load_lanelet_map(OSM, origin=(0.0, 0.0)), B, A, seed=0, device=dev)
    km = KinematicBicycle()
    km.set_params(lr=attributes[..., 2].contiguous())
    km.set_state(states)
    cfg = TorchDriveConfig(collision_metric=CollisionMetric.iou, renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(bench.RES, bench.RES), fov=bench.FOV)
    return Simulator(road, km, attributes[..., :2].contiguous(), placed, cfg, renderer=renderer)


def run_step(args):
    """a child process: one measurement, one JSON line"""
    import torch
    import bench
    from torchdrivesim_amd.utils import Resolution
    dev = torch.device('cuda', 0)
    B, A, R = args.batch, args.agents, args.rays
    sim = build(B, A, dev)
    extra = {}
    if args.step.startswith('scan'):
        kw = dict(n_rays=R, max_range=args.max_range, road=args.step != 'scan_agents_only', agents=args.step != 'scan_road_only')
        fn = lambda: sim.compute_range_scan(**kw)
        s = fn()
        extra = dict(values=3 * s.hit.numel(), bytes=12 * s.hit.numel(), mean_road_m=round(float(s.road.mean()), 3), mean_agents_m=round(float(s.agents.mean()), 3),
                     hit_entity=round(float((s.hit >= 0).float().mean()), 4), hit_road_edge=round(float((s.hit == -2).float().mean()), 4))
    elif args.step.startswith('render'):
        res = int(args.step.split('_')[1])
        out = torch.empty((B, A, 3, res, res), dtype=torch.float32, device=dev)
        fn = lambda: sim.render_egocentric(res=Resolution(res, res), fov=bench.FOV, out=out)
        extra = dict(bytes=out.numel() * 4)
    else:
        fn = lambda: (sim.compute_offroad(), sim.compute_collision())
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
    print(json.dumps(dict(step=args.step, reps=args.reps, warmup=args.warmup, ms_min=round(ms[0], 3), ms_median=round(ms[len(ms) // 2], 3), ms_max=round(ms[-1], 3),
                          device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip, **extra)), flush=True)


def kernel_trace(args, step):
    """one scan step under rocprofv3 --kernel-trace --stats -> the rows of its kernel statistics (most expensive first)"""
    out_dir = os.path.join(args.trace_dir, step)
    cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'scan', '--', sys.executable, os.path.abspath(__file__),
           '--step', step, '--batch', str(args.batch), '--agents', str(args.agents), '--rays', str(args.rays), '--max-range', str(args.max_range), '--reps', '10',
           '--warmup', '2']
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'trace of step {step} ended with status {done.returncode}: nothing more is started')
    rows, launch = trace_rows(out_dir)
    if not rows:
        sys.exit(f'trace of step {step}: rocprofv3 wrote no kernel statistics under {out_dir}')
    return keep_trace(args, step, rows, launch)


def trace_rows(out_dir):
    """the kernel statistics of a rocprofv3 run, most expensive first, in the columns of its *_kernel_stats.csv -- from that file, or, where the
    profiler kept its database instead (*_results.db), from the dispatch records in it; and the launch the profiler saw of range_scan_kernel"""
    found = sorted(glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True))
    if found:
        return list(csv.DictReader(open(found[0]))), None
    dbs = sorted(glob.glob(os.path.join(out_dir, '**', '*_results.db'), recursive=True))
    if not dbs:
        return [], None
    import sqlite3
    db = sqlite3.connect(dbs[0])
    per = {}
    for name, dur in db.execute('select name, duration from kernels'):
        per.setdefault(name, []).append(float(dur))
    total = sum(sum(v) for v in per.values())
    rows = []
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        mean = sum(v) / len(v)
        rows.append(dict(Name=name, Calls=str(len(v)), TotalDurationNs=str(int(sum(v))), AverageNs=f'{mean:.3f}', Percentage=f'{100 * sum(v) / total:.2f}',
                         MinNs=str(int(min(v))), MaxNs=str(int(max(v))), StdDev=f'{(sum((x - mean) ** 2 for x in v) / len(v)) ** 0.5:.3f}'))
    cur = db.execute("select grid_x, grid_y, workgroup_x, lds_size, scratch_size, vgpr_count, sgpr_count from kernels where name like '%range_scan_kernel%' limit 1")
    one = cur.fetchone()
    launch = None if one is None else dict(zip(('grid_x', 'grid_y', 'workgroup_x', 'lds_bytes', 'scratch_bytes', 'vgprs', 'sgprs'), one))
    return rows, launch


def keep_trace(args, step, rows, launch=None):
    keep = os.path.join(args.trace_dir, f'{step}_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/range_scan_timing.py --step {step} --reps 10 --warmup 2   (B = {args.batch} x A = {args.agents}, '
                f'{args.rays} rays, {args.max_range} m; the calls of the set-up -- map, spawn -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12]:
            w.writerow({k: (v if len(v) < 160 else v[:157] + '...') for k, v in r.items()})
    top = [dict(kernel=r['Name'].split('(')[0][-80:] if not r['Name'].startswith('(anonymous') else r['Name'].split('::', 1)[1].split('(')[0], calls=int(r['Calls']),
                total_ms=round(float(r['TotalDurationNs']) / 1e6, 3), mean_ms=round(float(r['AverageNs']) / 1e6, 4), min_ms=round(float(r['MinNs']) / 1e6, 4),
                max_ms=round(float(r['MaxNs']) / 1e6, 4), percent=round(float(r['Percentage']), 2)) for r in rows[:6]]
    return dict(step=step, stats_file=os.path.basename(keep), top_kernels=top, **({'range_scan_kernel_launch': launch} if launch else {}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--rays', type=int, default=64)
    ap.add_argument('--max-range', type=float, default=50.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'range_scan_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace the scan steps with rocprofv3 and keep their kernel statistics here')
    ap.add_argument('--step', choices=STEPS, help='(internal) run one measurement in this process')
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    rows = []
    for step in STEPS:
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(args.batch), '--agents', str(args.agents),
               '--rays', str(args.rays), '--max-range', str(args.max_range), '--reps', str(args.reps), '--warmup', str(args.warmup)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.exit(f'step {step} ended with status {done.returncode}: nothing more is started')
        rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    by = {r['step']: r for r in rows}
    doc = dict(date=datetime.date.today().isoformat(), device=rows[0]['device'], torch=rows[0]['torch'], hip=rows[0]['hip'], map='carla_Town01',
               batch=args.batch, agents=args.agents, rays=args.rays, max_range=args.max_range,
               what='HIP events around each call after warm-up, one child process per step; scan = torch.sin / torch.cos of the rays + one range_scan_kernel launch',
               scan_not_slower_than_render_64=by['scan']['ms_median'] <= by['render_64']['ms_median'], rows=rows)
    for r in rows:
        for k in ('device', 'torch', 'hip'):
            r.pop(k)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    def write():
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')

    write()
    if args.trace_dir:                                       # (the timings are on disk whatever the profiler does)
        os.makedirs(args.trace_dir, exist_ok=True)
        doc['kernel_trace'] = []
        for step in STEPS[:3]:
            doc['kernel_trace'].append(kernel_trace(args, step))
            print(json.dumps(doc['kernel_trace'][-1]), flush=True)
            write()
    print(json.dumps(dict(scan_ms=by['scan']['ms_median'], render_64_ms=by['render_64']['ms_median'], scan_not_slower_than_render_64=doc['scan_not_slower_than_render_64'])))


if __name__ == '__main__':
    main()
