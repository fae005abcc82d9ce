"""What giving way at junctions costs and does (behavior.LaneFollowingNPCController(give_way=True), csrc/conflicts.hip) on one MI355X.

Scene: Town01, B scenes x (A exposed agents + N NPCs) placed on the lanes by heuristic_initialize_batch.  Steps, each in a child process of its own
under `timeout` (the first that fails ends the run; nothing more is started on the device):
    advance     LaneFollowingNPCController.advance_npcs of two controllers over the same scene, one with the option and one without, called by
                turns; and the one-off build of the conflict table (tds_lane_conflicts_f64 into a tensor of its own, each call)
    rollout     --rollout-scenes x --rollout-npcs NPCs and nothing else over --rollout-steps steps, with and without the option: rectangle overlaps
                between NPCs per 1000 NPC-steps (tds_overlap_count_f32 on the NPC rows, a pair counted once) and the mean NPC speed
A timing: --warmup calls, then HIP events around each of --reps calls; min / median / max.  One run on one device: the figures say what this run
measured, not what every run will.

    python tools/give_way_timing.py [--batch 1024] [--agents 32] [--npcs 32] [--reps 20] [--warmup 3] [--out profiles/give_way_timing.json] [--trace-dir DIR]

--trace-dir: after the timed steps, advance_npcs with the option once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters),
its kernel statistics kept as DIR/give_way_kernel_stats.csv and their top rows copied into the JSON.
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
STEPS = ('advance', 'rollout', 'traced')
STEP_TIMEOUT_S = 400


def build(B, A, N, dev, give_way, agents_away=False):
    import torch
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.behavior import LaneFollowingNPCController, heuristic_initialize_batch
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    lanes = lanelet2.load_lanelet_map(OSM, origin=(0.0, 0.0))
    attributes, states, placed = heuristic_initialize_batch(lanes, B, A + N, seed=0, device=dev)
    if agents_away:                                                          # the exposed agents stand still: out of the NPCs' way
        states = states.clone()
        states[:, :A, :2] = 1.0e4
    km = KinematicBicycle()
    km.set_params(lr=attributes[:, :A, 2].contiguous())
    km.set_state(states[:, :A].contiguous())
    ctrl = LaneFollowingNPCController(lanes, attributes[:, A:, :2].contiguous(), states[:, A:].contiguous(), placed[:, A:].contiguous(), seed=1, give_way=give_way)
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    return Simulator(BirdviewMesh.empty(batch_size=B).to(dev), km, attributes[:, :A, :2].contiguous(), placed[:, :A].contiguous(), cfg, renderer=renderer,
                     npc_controller=ctrl, lanelet_map=[lanes] * B)


def timed(fns, reps, warmup):
    """the functions called by turns -> per function the sorted milliseconds of its `reps` calls"""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)] for _ in fns]
    for r in range(reps):
        for e, fn in zip(ev, fns):
            e[2 * r].record()
            fn()
            e[2 * r + 1].record()
    torch.cuda.synchronize()
    return [sorted(e[2 * r].elapsed_time(e[2 * r + 1]) for r in range(reps)) for e in ev]


def summary(ms):
    return dict(ms_min=round(ms[0], 4), ms_median=round(ms[len(ms) // 2], 4), ms_max=round(ms[-1], 4))


def run_step(args):
    """a child process: one measurement, one JSON line"""
    import torch
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    dev = torch.device('cuda', 0)
    versions = dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip)
    if args.step in ('advance', 'traced'):
        B, A, N = args.batch, args.agents, args.npcs
        sims = [build(B, A, N, dev, give_way=True)] + ([] if args.step == 'traced' else [build(B, A, N, dev, give_way=False)])
        ms = timed([lambda s=s: s.npc_controller.advance_npcs(s) for s in sims], args.reps, args.warmup)
        out = dict(step=args.step, reps=args.reps, warmup=args.warmup, with_option=summary(ms[0]))
        if args.step == 'advance':
            table = sims[0].npc_controller._lane_table_set().tables[0]
            L = table.n_lanelets

            def build_table():                                               # what _ops.lane_conflicts does the first time, into a tensor of its own
                nat.call('tds_lane_conflicts_f64', dev, table.handle, torch.empty((L * (L + 2),), dtype=torch.float64, device=dev), 2.0, 0.5)
            c = sims[0].npc_controller
            out.update(without_option=summary(ms[1]), ratio_of_medians=round(ms[0][len(ms[0]) // 2] / ms[1][len(ms[1]) // 2], 3),
                       table_build=summary(timed([build_table], args.reps, args.warmup)[0]), lanelets=L,
                       conflicting_pairs=int(((_ops.lane_conflicts(table)[0] >= 0) & (_ops.lane_conflicts(table)[0].T >= 0)).sum()),
                       npcs_giving_way=round(float((c.yield_to >= 0).float().mean()), 4))
        print(json.dumps(dict(out, **versions)), flush=True)
        return
    B, N = args.rollout_scenes, args.rollout_npcs
    out = dict(step='rollout', scenes=B, npcs=N, steps=args.rollout_steps)
    for give_way in (True, False):
        sim = build(B, 1, N, dev, give_way, agents_away=True)
        c = sim.npc_controller
        action = torch.zeros((B, 1, 2), device=dev)
        overlaps, speed = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
        for _ in range(args.rollout_steps):
            sim.step(action)
            boxes = torch.cat([c.npc_state[..., :2], c.npc_size, c.npc_state[..., 2:3]], dim=-1)
            overlaps += _ops.overlap_count(boxes, c.npc_present_mask, c.npc_sc).sum() / 2
            speed += c.npc_state[..., 3][c.npc_present_mask].double().mean()
        npc_steps = float(c.npc_present_mask.sum()) * args.rollout_steps
        out['with_option' if give_way else 'without_option'] = dict(
            overlaps_per_1000_npc_steps=round(1000.0 * float(overlaps) / npc_steps, 4), mean_speed=round(float(speed) / args.rollout_steps, 4),
            lanelet_changes=int(c.hops.sum()), standing_at_the_end=round(float((c.npc_state[..., 3][c.npc_present_mask] == 0).float().mean()), 4))
    print(json.dumps(dict(out, **versions)), flush=True)


def child(args, step, reps, warmup):
    return [sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(args.batch), '--agents', str(args.agents), '--npcs', str(args.npcs),
            '--reps', str(reps), '--warmup', str(warmup), '--rollout-scenes', str(args.rollout_scenes), '--rollout-npcs', str(args.rollout_npcs),
            '--rollout-steps', str(args.rollout_steps)]


def kernel_trace(args):
    """advance_npcs with the option under rocprofv3 --kernel-trace --stats -> the top rows of its kernel statistics"""
    import csv
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'traced')
    cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'give_way', '--'] + \
        child(args, 'traced', 10, 2)
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}: nothing more is started')
    rows, _ = trace_rows(out_dir)
    if not rows:
        sys.exit(f'rocprofv3 wrote no kernel statistics under {out_dir}')
    keep = os.path.join(args.trace_dir, 'give_way_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/give_way_timing.py --step traced --reps 10 --warmup 2   (B = {args.batch} x '
                f'(A = {args.agents} + N = {args.npcs}), give_way=True; the calls of the set-up -- lane and conflict tables, spawn, snap -- included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:12]:
            w.writerow({k: (v if len(v) < 160 else v[:157] + '...') for k, v in r.items()})
    short = lambda n: n.split('(')[0][-80:] if not n.startswith('(anonymous') else n.split('::', 1)[1].split('(')[0]
    return dict(stats_file=os.path.basename(keep),
                kernels=[dict(kernel=short(r['Name']), calls=int(r['Calls']), mean_ms=round(float(r['AverageNs']) / 1e6, 4), min_ms=round(float(r['MinNs']) / 1e6, 4),
                              max_ms=round(float(r['MaxNs']) / 1e6, 4)) for r in rows if any(k in r['Name'] for k in ('lane_give_way', 'lane_follow', 'lane_conflicts'))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=32)
    ap.add_argument('--npcs', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rollout-scenes', type=int, default=64)
    ap.add_argument('--rollout-npcs', type=int, default=32)
    ap.add_argument('--rollout-steps', type=int, default=3000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'give_way_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace advance_npcs with rocprofv3 and keep its kernel statistics here')
    ap.add_argument('--step', choices=STEPS, help='(internal) run one measurement in this process')
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    rows = []
    for step in ('advance', 'rollout'):
        done = subprocess.run(['timeout', '-k', '10', str(STEP_TIMEOUT_S)] + child(args, step, args.reps, args.warmup), capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stdout + done.stderr)
            sys.exit(f'step {step} ended with status {done.returncode}: nothing more is started')
        rows.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    doc = dict(date=datetime.date.today().isoformat(), device=rows[0]['device'], torch=rows[0]['torch'], hip=rows[0]['hip'], map='carla_Town01', batch=args.batch,
               agents=args.agents, npcs=args.npcs, runs='one run',
               what='HIP events around each call after warm-up, the two controllers called by turns; advance_npcs = the entity tensors (torch.cat), with the '
                    'option the red mask and one lane_give_way_kernel launch, then one lane_follow_kernel launch', rows=rows)
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
        doc['kernel_trace'] = kernel_trace(args)
        print(json.dumps(doc['kernel_trace']), flush=True)
        write()


if __name__ == '__main__':
    main()
