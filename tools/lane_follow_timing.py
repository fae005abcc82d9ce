"""Launch times of lane-following NPC traffic (behavior.LaneFollowingNPCController, csrc/follow.hip) on one MI355X, and in the SAME run the plain
Simulator.step it is added to.

Scene: Town01, B scenes x (A exposed agents + N NPCs) placed on the lanes by heuristic_initialize_batch.  Steps, each in a child process of its own
under `timeout` (the first that fails ends the run; nothing more is started on the device):
    advance_npcs        LaneFollowingNPCController.advance_npcs alone: the entity tensors (torch.cat) + one lane_follow_kernel launch
    step_with           a whole Simulator.step (random actions) with the controller
    step_without        the same scene with the base NPCController, whose NPCs stand still
A step: --warmup calls, then HIP events around each of --reps calls; min / median / max.  One run on one device: the figures say what this run
measured, not what every run will.

    python tools/lane_follow_timing.py [--batch 1024] [--agents 32] [--npcs 32] [--reps 20] [--warmup 3] [--out profiles/lane_follow_timing.json]
                                       [--trace-dir DIR]

--trace-dir: after the timed steps, advance_npcs once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters), its kernel
statistics kept as DIR/advance_npcs_kernel_stats.csv and their top rows copied into the JSON.
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
OSM = os.path.join(ROOT, 'tests', 'golden', 'carla_Town01.osm.gz')
STEPS = ('advance_npcs', 'step_with', 'step_without')
STEP_TIMEOUT_S = 240


def build(B, A, N, dev, follow):
    import torch
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.behavior import LaneFollowingNPCController, heuristic_initialize_batch
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import NPCController, Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    lanes = lanelet2.load_lanelet_map(OSM, origin=(0.0, 0.0))
    attributes, states, placed = heuristic_initialize_batch(lanes, B, A + N, seed=0, device=dev)
    km = KinematicBicycle()
    km.set_params(lr=attributes[:, :A, 2].contiguous())
    km.set_state(states[:, :A].contiguous())
    npc = (attributes[:, A:, :2].contiguous(), states[:, A:].contiguous(), placed[:, A:].contiguous())
    ctrl = LaneFollowingNPCController(lanes, *npc, seed=1) if follow else NPCController(*npc)
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    return Simulator(BirdviewMesh.empty(batch_size=B).to(dev), km, attributes[:, :A, :2].contiguous(), placed[:, :A].contiguous(), cfg, renderer=renderer,
                     npc_controller=ctrl, lanelet_map=[lanes] * B)


def run_step(args):
    """a child process: one measurement, one JSON line"""
    import torch
    dev = torch.device('cuda', 0)
    B, A, N = args.batch, args.agents, args.npcs
    sim = build(B, A, N, dev, follow=args.step != 'step_without')
    g = torch.Generator(device=dev).manual_seed(0)
    action = torch.rand((B, A, 2), device=dev, generator=g) * 2 - 1
    fn = (lambda: sim.npc_controller.advance_npcs(sim)) if args.step == 'advance_npcs' else (lambda: sim.step(action))
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
    extra = {}
    if args.step != 'step_without':
        c = sim.npc_controller
        extra = dict(npcs_on_a_lane=round(float((c.lane >= 0).float().mean()), 4), npcs_behind_a_leader=round(float((c.leader >= 0).float().mean()), 4),
                     mean_speed=round(float(c.npc_state[..., 3].mean()), 3), hops=int(c.hops.sum()))
    print(json.dumps(dict(step=args.step, reps=args.reps, warmup=args.warmup, ms_min=round(ms[0], 3), ms_median=round(ms[len(ms) // 2], 3), ms_max=round(ms[-1], 3),
                          device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip, **extra)), flush=True)


def child(args, step, reps, warmup):
    return [sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(args.batch), '--agents', str(args.agents), '--npcs', str(args.npcs),
            '--reps', str(reps), '--warmup', str(warmup)]


def kernel_trace(args, step):
    """one step under rocprofv3 --kernel-trace --stats -> the top rows of its kernel statistics"""
    import csv
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, step)
    cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'follow', '--'] + \
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
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/lane_follow_timing.py --step {step} --reps 10 --warmup 2   (B = {args.batch} x '
                f'(A = {args.agents} + N = {args.npcs}); the calls of the set-up -- lane tables, spawn, snap -- included)\n')
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
    ap.add_argument('--agents', type=int, default=32)
    ap.add_argument('--npcs', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lane_follow_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace advance_npcs with rocprofv3 and keep its kernel statistics here')
    ap.add_argument('--step', choices=STEPS, help='(internal) run one measurement in this process')
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    rows = []
    for step in STEPS:
        done = subprocess.run(['timeout', '-k', '10', str(STEP_TIMEOUT_S)] + child(args, step, args.reps, args.warmup), capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.exit(f'step {step} ended with status {done.returncode}: nothing more is started')
        rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    by = {r['step']: r for r in rows}
    doc = dict(date=datetime.date.today().isoformat(), device=rows[0]['device'], torch=rows[0]['torch'], hip=rows[0]['hip'], map='carla_Town01',
               batch=args.batch, agents=args.agents, npcs=args.npcs,
               what='HIP events around each call after warm-up, one child process per step; advance_npcs = the entity tensors (torch.cat) + one lane_follow_kernel launch',
               npcs_cost_more_than_the_rest_of_the_step=by['advance_npcs']['ms_median'] > by['step_without']['ms_median'], rows=rows)
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
        doc['kernel_trace'] = [kernel_trace(args, 'advance_npcs')]
        print(json.dumps(doc['kernel_trace'][-1]), flush=True)
        write()
    print(json.dumps(dict(advance_npcs_ms=by['advance_npcs']['ms_median'], step_with_ms=by['step_with']['ms_median'], step_without_ms=by['step_without']['ms_median'])))


if __name__ == '__main__':
    main()
