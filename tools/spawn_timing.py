"""Launch times of the on-lane initialisation (`heuristic_initialize_batch`, csrc/spawn.hip) on one MI355X, and beside them the time of the
only path a user had before it: the host loop of the same algorithm -- one point query and one disc test per attempt, as tests/spawn_model.py
runs it -- on a bounded sample of the same scenes, spread over the CPUs this process may use.

Device: Town01, B scenes x A agents, HIP events around each of --reps launches after --warmup, a NEW seed every repetition (the work of a
launch depends on the draw), median and range reported.  Writes one JSON document (--out) and prints it.

    python tools/spawn_timing.py [--batch 1024] [--agents 64 256] [--reps 20] [--warmup 3] [--host-scenes 64] [--out profiles/spawn_timing.json]
"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OSM = os.path.join(ROOT, 'tests', 'golden', 'carla_Town01.osm.gz')


def _host_scenes(job):
    """a worker process: the model's loop over its share of the scenes (no GPU in here)"""
    import spawn_model as sm
    from oracle import oracle as orc
    from torchdrivesim_amd import lanelet2
    seed, scene_ids, agents = job
    lanes = sm.Lanes(lanelet2.lane_table(lanelet2.load_lanelet_map(OSM, origin=(0.0, 0.0))))
    t0 = time.perf_counter()
    attempts = 0
    for s in scene_ids:
        attempts += int(sm.spawn_scene(orc, lanes, seed, s, sm.default_attributes(agents))[3].sum())
    return time.perf_counter() - t0, attempts


def host_loop(agents, n_scenes, seed):
    from oracle import oracle as orc
    orc.build()
    workers = min(orc.usable_cpus(), n_scenes)
    shares = [list(range(w, n_scenes, workers)) for w in range(workers)]
    t0 = time.perf_counter()
    with concurrent.futures.ProcessPoolExecutor(workers) as pool:
        done = list(pool.map(_host_scenes, [(seed, share, agents) for share in shares]))
    wall = time.perf_counter() - t0
    busy = max(d[0] for d in done)              # the slowest worker, without process start-up and map loading: the time `workers` CPUs need
    return dict(scenes=n_scenes, workers=workers, wall_s=round(wall, 3), loop_s=round(busy, 3), ms_per_scene=round(1e3 * busy / n_scenes, 3), ms_per_scene_one_cpu=round(1e3 * sum(d[0] for d in done) / n_scenes, 3),
                attempts_per_agent=round(sum(d[1] for d in done) / (n_scenes * agents), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-scenes', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spawn_timing.json'))
    args = ap.parse_args()
    # the host loop first, in worker processes started before this process touches the GPU
    host = {A: host_loop(A, args.host_scenes, seed=1) for A in args.agents} if args.host_scenes > 0 else {}
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    dev = torch.device('cuda', 0)
    lanes = lanelet2.load_lanelet_map(OSM, origin=(0.0, 0.0))
    rows = []
    for A in args.agents:
        B = args.batch
        for w in range(args.warmup):
            heuristic_initialize_batch(lanes, B, A, seed=1000 + w, on_failure='mask', device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.reps)]
        placed = []
        for r in range(args.reps):
            ev[2 * r].record()
            placed.append(heuristic_initialize_batch(lanes, B, A, seed=r, on_failure='mask', device=dev)[2])
            ev[2 * r + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(args.reps))
        row = dict(batch=B, agents=A, reps=args.reps, ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3), ms_max=round(ms[-1], 3),
                   all_placed=bool(all(bool(p.all()) for p in placed)), host_loop=host.get(A))
        if host.get(A):
            row['host_loop_ms_for_this_batch'] = round(host[A]['ms_per_scene'] * B, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = dict(device=torch.cuda.get_device_name(dev), map='carla_Town01', what='heuristic_initialize_batch(on_failure="mask"): attribute fills + one '
               'spawn_on_lanes_kernel launch per call, HIP events, a new seed per repetition', rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
