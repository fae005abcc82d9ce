"""Times of the traffic lights on the device (traffic_controls.ProgrammedTrafficLightControl, Simulator.compute_stop_lines; csrc/lights.hip) on one
MI355X, and in the SAME run what they are to be weighed against:

    host_shared        the host path of examples/step_loop.py: ONE host controller ticked, one index tensor built, expanded and copied to the device
    host_per_scene_64  64 host controllers ticked and their 64 index tensors stacked and copied; `host_per_scene_extrapolated` is that x B / 64
    device_tick        ProgrammedTrafficLightControl.tick(0.1): B clocks of their own, one launch
    device_reset       ProgrammedTrafficLightControl.reset(): two launches
    stop_lines         Simulator.compute_stop_lines(k=4)         beside    neighbors    Simulator.compute_neighbors(k=8)
    step_host          host_shared + Simulator.step              beside    step_device  Simulator.step with the programmed control

Scene: Town01 (12 machines, 36 lights), B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch.  One child process under
`timeout` measures: --warmup calls of each, then HIP events around each of --reps calls -- the events are on the stream, so the host's own work
between them counts --, all taking turns within every repeat; min / median / max.  One run on one device: the figures say what this run
measured, not what every run will.

    python tools/lights_timing.py [--batch 1024] [--agents 64] [--reps 20] [--warmup 3] [--out profiles/lights_timing.json] [--trace-dir DIR]

--trace-dir: afterwards tick, reset and compute_stop_lines alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters);
the kernel statistics are kept as DIR/lights_kernel_stats.csv and the rows of the three kernels go into the JSON: the time per dispatch.
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
KERNELS = ('lights_step_kernel', 'lights_reset_kernel', 'stop_lines_kernel')


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import range_scan_timing
    from route_to_timing import timed
    from torchdrivesim_amd.map import load_map_config, programmed_traffic_lights_from_map_config, traffic_controls_from_map_config
    from torchdrivesim_amd.traffic_lights import current_light_state_tensor_from_controller as colours
    dev = torch.device('cuda', 0)
    B, A = args.batch, args.agents
    sim = range_scan_timing.build(B, A, dev)
    cfg = load_map_config(PACKAGE)
    ids = [s.actor_id for s in cfg.stoplines if s.agent_type == 'traffic_light']
    programmed = programmed_traffic_lights_from_map_config(cfg, B, dev, dt=0.1, seed=0)
    sim.traffic_controls = {'traffic_light': programmed}
    fns = dict(device_tick=lambda: programmed.tick(0.1), device_reset=lambda: programmed.reset(),
               stop_lines=lambda: sim.compute_stop_lines(k=4))
    if not args.only_device:
        plain = traffic_controls_from_map_config(cfg)['traffic_light'].extend(B).to(dev)
        shared = cfg.traffic_light_controller
        many = [cfg.traffic_light_controller for _ in range(64)]
        action = torch.zeros((B, A, 2), device=dev)

        def host_shared():
            shared.tick(0.1)
            plain.set_state(colours(shared, ids).unsqueeze(0).expand(B, -1).to(dev))

        def host_per_scene_64():
            for c in many:
                c.tick(0.1)
            return torch.stack([colours(c, ids) for c in many]).to(dev)

        def step_with(control, before=None):
            def fn():
                sim.traffic_controls = {'traffic_light': control}
                if before is not None:
                    before()
                sim.step(action)
            return fn
        fns.update(host_shared=host_shared, host_per_scene_64=host_per_scene_64, neighbors=lambda: sim.compute_neighbors(k=8),
                   step_host=step_with(plain, host_shared), step_device=step_with(programmed))
    ms = timed(fns, args.reps, args.warmup)
    sim.traffic_controls = {'traffic_light': programmed}
    sl = sim.compute_stop_lines(k=4)
    rows = []
    for step, m in ms.items():
        rows.append(dict(step=step, reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4)))
        if step == 'stop_lines':
            rows[-1].update(bytes=sl.features.numel() * 4 + sl.index.numel() * 8, filled_slots=round(float(sl.mask.float().mean()), 4))
    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip, machines=int(programmed.phase.shape[1]),
                          lights=len(ids), rows=rows)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--reps', str(reps or args.reps),
            '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """tick, reset and compute_stop_lines alone under rocprofv3 --kernel-trace --stats -> the statistics of the three kernels"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'lights')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'lights', '--',
           *child(args, '--only-device', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = [r for r in rows if any(k in r['Name'] for k in KERNELS)]
    if len(mine) != len(KERNELS):
        sys.exit(f'the trace under {out_dir} does not hold {KERNELS}')
    keep = os.path.join(args.trace_dir, 'lights_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/lights_timing.py --measure --only-device --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, Town01; the calls of the set-up -- spawn -- included)\n')
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lights_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace the three kernels with rocprofv3 and keep their statistics here')
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    ap.add_argument('--only-device', action='store_true', help='(internal) tick, reset and compute_stop_lines alone')
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
    doc = dict(date=datetime.date.today().isoformat(), device=got['device'], torch=got['torch'], hip=got['hip'], map='carla_Town01', batch=args.batch,
               agents=args.agents, machines=got['machines'], lights=got['lights'],
               what='HIP events on the stream around each call after warm-up (the host\'s work between them counts), all in one process; the calls take '
                    'turns within every repeat',
               host_per_scene_extrapolated=dict(ms_median=round(med('host_per_scene_64') * args.batch / 64, 3),
                                                note=f'EXTRAPOLATED: the median of 64 host controllers x {args.batch} / 64; not measured at {args.batch}'),
               device_tick_over_host_shared=round(med('device_tick') / med('host_shared'), 5),
               expectation_tick_not_slower_than_the_shared_host_clock_met=med('device_tick') <= med('host_shared'),
               stop_lines_over_neighbors=round(med('stop_lines') / med('neighbors'), 5),
               expectation_stop_lines_within_2x_of_neighbors_met=med('stop_lines') <= 2.0 * med('neighbors'),
               step_device_over_step_host=round(med('step_device') / med('step_host'), 5), rows=got['rows'])

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
