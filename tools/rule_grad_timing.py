"""Launch times of the gradients of the rule terms -- Simulator.compute_stop_lines(differentiable=True) (K7b, csrc/stop_lines_bwd.hip) and
Simulator.compute_wrong_way(differentiable=True) (tds_wrong_way_grad_f32, csrc/lanes.hip) -- on one MI355X, and in the SAME run what they are to
be weighed against: today's calls and launches, and the backward launch of the neighbour observations (K6b) at the same B, A and K.

Scene: Town01 with programmed lights, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch (the scene of
tools/lights_timing.py), every other agent turned by 2.6 rad so that it drives against its lane.  One child process under `timeout` measures, taking turns call by call, for k = 4 and k = 8:
    stop_lines_call / _differentiable   compute_stop_lines as it always was / with differentiable=True on a state that requires grad
    stop_lines_forward_launch           tds_stop_lines_f32 alone
    stop_lines_backward_launch          tds_stop_lines_bwd_f32 alone, a random incoming gradient: the product's launch, 4 lanes per observer
    stop_lines_backward_lanes_16/4/1    the same entry point of the testing build with 16, 4 and 1 lanes per observer (16: K6b's shape; 1: a thread per observer): the shapes weighed against each other
    neighbors_backward_launch           tds_neighbors_bwd_f32 alone on the index of its own forward (E = A entities), a random gradient
and once:
    wrong_way_call / _differentiable    compute_wrong_way as it always was / with differentiable=True on a state that requires grad
    wrong_way_launch                    tds_wrong_way_f32 alone
    wrong_way_grad_launch               tds_wrong_way_grad_f32 alone: the same kernel with one more pointer
--warmup rounds, then HIP events around each call of --reps rounds; median (min - max).  The expectations to report against: the K7b launch is no
slower than the K6b launch of the same run, the margin being that launch's own min-max spread; the wrong-way launch that also writes the
derivative is no slower than today's, within that launch's spread.  One run on one device: the figures say what this run measured, not what every
run will.

    python tools/rule_grad_timing.py [--batch 1024] [--agents 64] [--reps 20] [--warmup 3] [--out profiles/rule_grad_timing.json] [--trace-dir DIR]

--trace-dir: afterwards the launches alone once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the kernel
statistics are kept as DIR/rule_grad_kernel_stats.csv and the rows of the kernels go into the JSON: the time per dispatch.
"""
import argparse
import csv
import datetime
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
KS = (4, 8)
TIMEOUT_S = 500
KERNELS = ('stop_lines_kernel', r'stop_lines_bwd_kernel<4>', 'neighbors_bwd_kernel', 'wrong_way_kernel')
REACH = 60.0


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import lights_timing
    import range_scan_timing
    from route_to_timing import timed
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops, lanelet2
    from torchdrivesim_amd.map import load_map_config, programmed_traffic_lights_from_map_config
    dev = torch.device('cuda', 0)
    B, A = args.batch, args.agents
    sim = range_scan_timing.build(B, A, dev)
    sim.lanelet_map = [lanelet2.load_lanelet_map(range_scan_timing.OSM, origin=(0.0, 0.0))] * B
    control = programmed_traffic_lights_from_map_config(load_map_config(lights_timing.PACKAGE), B, dev, dt=0.1, seed=0)
    sim.traffic_controls = {'traffic_light': control}
    plain = sim.get_state().detach().clone()
    plain[:, 1::2, 2] += 2.6                                 # every other agent drives against its lane: the wrong-way loss has something to say
    sim.kinematic_model.set_state(plain)
    leaf = plain.detach().clone().requires_grad_(True)
    st = plain.detach()
    xy, sc = st[..., :2].contiguous(), _ops.heading_sc(st[..., 2]).contiguous()
    present = _ops._u8(sim.get_present_mask())
    lines = control.pos.contiguous()
    line_sc, mask, N = _ops.heading_sc(lines[..., 4]).contiguous(), _ops._u8(control.mask), lines.shape[1]
    boxes = torch.cat([st[..., :2], sim.get_agent_size(), st[..., 2:3]], -1).contiguous()
    speed = st[..., 3].contiguous()
    gen = torch.Generator(device=dev).manual_seed(0)
    lane_set = sim._lane_tables(dev)
    tol, thr = sim.cfg.lanelet_inclusion_tolerance, sim.cfg.wrong_way_angle_threshold
    out, out2, dpsi = (torch.empty((B, A), device=dev) for _ in range(3))
    fns, per_k = {}, {}

    def with_state(state, fn):
        def run():
            sim.kinematic_model.set_state(state)
            return fn()
        return run

    for K in KS:
        t = dict(features=torch.empty((B, A, K, 8), device=dev), index=torch.empty((B, A, K), dtype=torch.int32, device=dev),
                 slot_state=torch.empty((B, A, K), dtype=torch.int32, device=dev), g=torch.randn((B, A, K, 8), device=dev, generator=gen),
                 g_xy=torch.empty((B, A, 2), device=dev), g_sc=torch.empty((B, A, 2), device=dev), nb_features=torch.empty((B, A, K, 8), device=dev),
                 nb_index=torch.empty((B, A, K), dtype=torch.int32, device=dev), g_boxes=torch.empty((B, A, 5), device=dev),
                 nb_g_sc=torch.empty((B, A, 2), device=dev), g_speed=torch.empty((B, A), device=dev))
        per_k[K] = t

        def forward(t=t, K=K):
            nat.call('tds_stop_lines_f32', dev, xy, sc, present, lines, line_sc, mask, control.state, control.time_to_change, t['features'], t['index'],
                     t['slot_state'], B, A, N, K, REACH, 1, float('-inf'))

        def backward(t=t, K=K):
            nat.call('tds_stop_lines_bwd_f32', dev, xy, sc, lines, line_sc, t['index'], t['g'], t['g_xy'], t['g_sc'], B, A, N, K)

        def backward_lanes(lanes, t=t, K=K):
            def run():
                with nat.testing() as lib:
                    nat.check(lib.tds_stop_lines_bwd_set_row_lanes(lanes), 'tds_stop_lines_bwd_set_row_lanes')
                    nat.call('tds_stop_lines_bwd_f32', dev, xy, sc, lines, line_sc, t['index'], t['g'], t['g_xy'], t['g_sc'], B, A, N, K)
            return run

        def neighbors_backward(t=t, K=K):
            nat.call('tds_neighbors_bwd_f32', dev, boxes, sc, speed, t['nb_index'], t['g'], t['g_boxes'], t['nb_g_sc'], t['g_speed'], B, A, A, K)

        forward()                                            # the indices exist before the backwards are first warmed up
        nat.call('tds_neighbors_f32', dev, boxes, sc, speed, present, None, t['nb_features'], t['nb_index'], B, A, A, K, 50.0)
        fns.update({f'stop_lines_forward_launch_k{K}': forward, f'stop_lines_backward_launch_k{K}': backward,
                    f'neighbors_backward_launch_k{K}': neighbors_backward})
        if not args.only_launches:
            fns.update({f'stop_lines_backward_lanes_{n}_k{K}': backward_lanes(n) for n in (16, 4, 1)})
            fns.update({f'stop_lines_call_k{K}': with_state(plain, lambda K=K: sim.compute_stop_lines(k=K, max_distance=REACH)),
                        f'stop_lines_call_differentiable_k{K}': with_state(leaf, lambda K=K: sim.compute_stop_lines(k=K, max_distance=REACH, differentiable=True))})

    def wrong_way_launch():
        nat.call('tds_wrong_way_f32', dev, lane_set.handle, lane_set.scene_map, A, st, None, present, out, B * A, thr, tol)

    def wrong_way_grad_launch():
        nat.call('tds_wrong_way_grad_f32', dev, lane_set.handle, lane_set.scene_map, A, st, None, present, out2, dpsi, B * A, thr, tol)

    fns.update(wrong_way_launch=wrong_way_launch, wrong_way_grad_launch=wrong_way_grad_launch)
    if not args.only_launches:
        fns.update(wrong_way_call=with_state(plain, sim.compute_wrong_way),
                   wrong_way_call_differentiable=with_state(leaf, lambda: sim.compute_wrong_way(differentiable=True)))
    ms = timed(fns, args.reps, args.warmup)
    rows = [dict(step=name, reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4))
            for name, m in ms.items()]
    for K in KS:                                             # what was timed did something
        t = per_k[K]
        fns[f'stop_lines_backward_launch_k{K}']()
        fns[f'neighbors_backward_launch_k{K}']()
        torch.cuda.synchronize()
        assert bool((t['g_xy'] != 0).any()) and bool((t['index'] >= 0).any()) and bool((t['g_boxes'] != 0).any())
    wrong_way_launch()
    wrong_way_grad_launch()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and bool((dpsi != 0).any())
    sim.kinematic_model.set_state(plain)
    filled = {f'stop_line_slots_filled_k{K}': round(float((per_k[K]['index'] >= 0).float().mean()), 4) for K in KS}
    filled.update({f'neighbor_slots_filled_k{K}': round(float((per_k[K]['nb_index'] >= 0).float().mean()), 4) for K in KS})
    print(json.dumps(dict(rows=rows, lines=int(N), agents_with_a_wrong_way_loss=round(float((out > 0).float().mean()), 4),
                          agents_with_a_derivative=round(float((dpsi != 0).float().mean()), 4), **filled, device=torch.cuda.get_device_name(dev),
                          torch=torch.__version__, hip=torch.version.hip)), flush=True)


def child(args, *extra, reps=None, warmup=None):
    return [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--reps', str(reps or args.reps),
            '--warmup', str(warmup or args.warmup), *extra]


def kernel_trace(args):
    """the launches alone under rocprofv3 --kernel-trace --stats -> the statistics of their kernels"""
    from range_scan_timing import trace_rows
    out_dir = os.path.join(args.trace_dir, 'rule_grad')
    cmd = ['timeout', '-k', '10', str(TIMEOUT_S), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'rule_grad', '--',
           *child(args, '--only-launches', reps=10, warmup=2)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the trace ended with status {done.returncode}')
    rows, _ = trace_rows(out_dir)
    mine = {k: [r for r in rows if re.search(r'(?<![A-Za-z0-9_])' + re.escape(k) + r'(?![A-Za-z0-9_])', r['Name'])] for k in KERNELS}        # the whole name
    if not all(mine.values()):
        sys.exit(f'the trace under {out_dir} does not hold all of {KERNELS}')
    keep = os.path.join(args.trace_dir, 'rule_grad_kernel_stats.csv')
    with open(keep, 'w') as f:
        f.write(f'# rocprofv3 --kernel-trace --stats --output-format csv -- python tools/rule_grad_timing.py --measure --only-launches --reps 10 --warmup 2   '
                f'(B = {args.batch} x A = {args.agents}, k = 4 and k = 8 in the same rows; wrong_way_kernel: both entry points; the calls of the set-up included)\n')
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        w.writeheader()
        for r in rows[:14]:
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rule_grad_timing.json'))
    ap.add_argument('--trace-dir', default=None, help='also trace the launches with rocprofv3 and keep their kernel statistics here')
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    ap.add_argument('--only-launches', action='store_true', help='(internal) the launches of the product alone')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    done = subprocess.run(['timeout', '-k', '10', str(TIMEOUT_S), *child(args)], capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    rows = got.pop('rows')
    by = {r['step']: r for r in rows}
    ratios = {}
    for K in KS:
        bwd, nb = by[f'stop_lines_backward_launch_k{K}'], by[f'neighbors_backward_launch_k{K}']
        margin = round(nb['ms_max'] - nb['ms_min'], 4)
        ratios[f'k{K}'] = dict(
            stop_lines_backward_over_neighbors_backward=round(bwd['ms_median'] / nb['ms_median'], 3), margin_ms_neighbors_backward_spread=margin,
            expectation_no_slower_than_neighbors_backward_met=bwd['ms_median'] <= nb['ms_median'] + margin,
            stop_lines_backward_over_forward=round(bwd['ms_median'] / by[f'stop_lines_forward_launch_k{K}']['ms_median'], 3),
            lanes_16_over_lanes_4=round(by[f'stop_lines_backward_lanes_16_k{K}']['ms_median'] / by[f'stop_lines_backward_lanes_4_k{K}']['ms_median'], 3),
            lanes_1_over_lanes_4=round(by[f'stop_lines_backward_lanes_1_k{K}']['ms_median'] / by[f'stop_lines_backward_lanes_4_k{K}']['ms_median'], 3),
            call_differentiable_over_call=round(by[f'stop_lines_call_differentiable_k{K}']['ms_median'] / by[f'stop_lines_call_k{K}']['ms_median'], 3))
    ww, wwg = by['wrong_way_launch'], by['wrong_way_grad_launch']
    margin = round(ww['ms_max'] - ww['ms_min'], 4)
    ratios['wrong_way'] = dict(grad_launch_over_launch=round(wwg['ms_median'] / ww['ms_median'], 3), margin_ms_launch_spread=margin,
                               expectation_grad_launch_no_slower_met=wwg['ms_median'] <= ww['ms_median'] + margin,
                               call_differentiable_over_call=round(by['wrong_way_call_differentiable']['ms_median'] / by['wrong_way_call']['ms_median'], 3))
    doc = dict(date=datetime.date.today().isoformat(), device=got.pop('device'), torch=got.pop('torch'), hip=got.pop('hip'), map='carla_Town01', batch=args.batch,
               agents=args.agents, k=list(KS), max_distance=REACH,
               what='HIP events around each call after warm-up, ONE process, all calls taking turns; the `_call`, `stop_lines_forward_launch`, '
                    '`neighbors_backward_launch` and `wrong_way_launch` rows are the code paths of the parent commit, measured again in this run; the '
                    '`_lanes_` rows go through the testing build of the library, which sets the lanes per observer before each launch.  Measured: the '
                    'host-side launches and their kernels as the events see them.  Not measured: a loss and autograd\'s walk to the backward nodes, the '
                    'contiguous copies the stop-line backward node makes of `state[..., :2]` and, where it is strided or misaligned, of the incoming '
                    'gradient before its one launch, the torch product of the wrong-way backward, hardware counters, any other scene, K, line count or agent count',
               **got, ratios=ratios, rows=rows)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')

    write()
    print(json.dumps({r['step']: f"{r['ms_median']} ({r['ms_min']} - {r['ms_max']})" for r in rows}), flush=True)
    print(json.dumps(ratios), flush=True)
    if args.trace_dir:                                       # (the timings are on disk whatever the profiler does)
        os.makedirs(args.trace_dir, exist_ok=True)
        doc['kernel_trace'] = kernel_trace(args)
        write()
        print(json.dumps(doc['kernel_trace']), flush=True)


if __name__ == '__main__':
    main()
