"""Launch times of the differentiable range scans (Simulator.compute_range_scan(differentiable=True), csrc/scan_bwd.hip) on one MI355X, and in the
SAME run what they are to be weighed against: the forward launch at the same B, A, E and R -- code this feature leaves as it was.

Scene: Town01, B scenes x A exposed agents placed on the lanes by heuristic_initialize_batch (the scene of tools/range_scan_timing.py).  One child
process under `timeout` measures, taking turns call by call:
    forward_launch          tds_range_scan_f32 alone, all three outputs: the range_scan_kernel launch
    backward_launch         tds_range_scan_bwd_f32 alone on the forward's road ranges, random incoming gradients: the range_scan_bwd_kernel launch
    forward_launch_agents   the forward without a map (road=False)
    backward_launch_agents  the backward without a map
--warmup rounds, then HIP events around each call of --reps rounds; median (min - max).  The expectations to report against: the full backward
launch is no slower than the full forward launch of the same run, the margin being that launch's own min-max spread (it replaces a walk over
the map by one lookup); the agents-only backward launch takes no more than 2 x the agents-only forward launch.  Neither is asserted anywhere.
One run on one device: the figures say what this run measured, not what every run will.

    python tools/range_scan_grad_timing.py [--batch 1024] [--agents 64] [--rays 64] [--max-range 50] [--reps 20] [--warmup 3]
                                           [--out profiles/range_scan_grad_timing.json]
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
STEPS = ('forward_launch', 'backward_launch', 'forward_launch_agents', 'backward_launch_agents')
TIMEOUT_S = 400
GAP = 0.02


def measure(args):
    """the child process: every measurement, one JSON line"""
    import torch
    import range_scan_timing
    from route_to_timing import timed
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import _static_maps_for
    dev = torch.device('cuda', 0)
    B, A, R = args.batch, args.agents, args.rays
    sim = range_scan_timing.build(B, A, dev)
    st = sim.get_state().detach()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1).contiguous()
    sc, present = _ops.heading_sc(st[..., 2]).contiguous(), _ops._u8(sim.get_all_agent_present_mask())
    ray_sc = _ops.heading_sc(st[..., 2].unsqueeze(-1) + sim.range_scan_angles(R, device=dev)).contiguous()
    smap = _static_maps_for(sim.road_mesh, dev)
    E = boxes.shape[1]
    gen = torch.Generator(device=dev).manual_seed(0)
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    agents, road, hit = new(B, A, R), new(B, A, R), new(B, A, R, dtype=torch.int32)
    agents0, road0, hit0 = new(B, A, R), new(B, A, R), new(B, A, R, dtype=torch.int32)
    g_agent, g_road = torch.randn((B, A, R), device=dev, generator=gen), torch.randn((B, A, R), device=dev, generator=gen)
    outs = [new(B, E, 5), new(B, E, 2), new(B, A, R, 2)]
    outs0 = [new(B, E, 5), new(B, E, 2), new(B, A, R, 2)]
    tail = (B, A, E, R, args.max_range, GAP)

    def forward_launch():
        nat.call(*_ops._map_head('tds_range_scan', '_f32', smap, dev), boxes, sc, present, ray_sc, agents, road, hit, *tail)

    def backward_launch():
        nat.call(*_ops._map_head('tds_range_scan_bwd', '_f32', smap, dev), boxes, sc, present, ray_sc, road, g_agent, g_road, *outs, None, None, *tail)

    def forward_launch_agents():
        nat.call('tds_range_scan_f32', dev, None, boxes, sc, present, ray_sc, agents0, road0, hit0, *tail)

    def backward_launch_agents():
        nat.call('tds_range_scan_bwd_f32', dev, None, boxes, sc, present, ray_sc, None, g_agent, None, *outs0, None, None, *tail)

    forward_launch()                                         # the road ranges exist before the backward is first warmed up
    ms = timed(dict(forward_launch=forward_launch, backward_launch=backward_launch, forward_launch_agents=forward_launch_agents,
                    backward_launch_agents=backward_launch_agents), args.reps, args.warmup)
    rows = [dict(step=name, reps=args.reps, warmup=args.warmup, ms_min=round(m[0], 4), ms_median=round(m[len(m) // 2], 4), ms_max=round(m[-1], 4))
            for name, m in ms.items()]
    torch.cuda.synchronize()
    live_agent = (agents > 0) & (agents < args.max_range)
    live_road = (road > 0) & (road < args.max_range)
    assert bool((outs[0] != 0).any()) and bool((outs0[0] != 0).any()) and bool(live_road.any())
    print(json.dumps(dict(rows=rows, rays_total=int(hit.numel()), rays_contributing_agents=round(float(live_agent.float().mean()), 4),
                          rays_contributing_road=round(float(live_road.float().mean()), 4),
                          rays_contributing=round(float((live_agent | live_road).float().mean()), 4), mean_road_range_m=round(float(road.mean()), 2),
                          entities_with_a_gradient=round(float((outs[0][..., :4] != 0).any(-1).float().mean()), 4), entities=int(E),
                          device=torch.cuda.get_device_name(dev), torch=torch.__version__, hip=torch.version.hip)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--rays', type=int, default=64)
    ap.add_argument('--max-range', type=float, default=50.0)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'range_scan_grad_timing.json'))
    ap.add_argument('--measure', action='store_true', help='(internal) measure in this process')
    args = ap.parse_args()
    if args.measure:
        return measure(args)
    cmd = [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(args.batch), '--agents', str(args.agents), '--rays', str(args.rays),
           '--max-range', str(args.max_range), '--reps', str(args.reps), '--warmup', str(args.warmup)]
    done = subprocess.run(['timeout', '-k', '10', str(TIMEOUT_S), *cmd], capture_output=True, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-4000:] + done.stderr[-4000:])
        sys.exit(f'the measurement ended with status {done.returncode}')
    got = json.loads(done.stdout.strip().splitlines()[-1])
    by = {r['step']: r for r in got.pop('rows')}
    fwd, bwd, fwd0, bwd0 = (by[k] for k in STEPS)
    margin = round(fwd['ms_max'] - fwd['ms_min'], 4)
    doc = dict(date=datetime.date.today().isoformat(), device=got.pop('device'), torch=got.pop('torch'), hip=got.pop('hip'), map='carla_Town01', batch=args.batch,
               agents=args.agents, rays=args.rays, max_range=args.max_range, gap_tolerance=GAP,
               what='HIP events around each call after warm-up, ONE process, the four calls taking turns; the two forward launches are the code paths of '
                    'the parent commit, measured again in this run.  Measured: the host-side launches and their kernels as the events see them.  Not '
                    'measured: a loss and autograd\'s walk to the backward node, hardware counters, any other scene, ray or entity count',
               **got, backward_launch_over_forward_launch=round(bwd['ms_median'] / fwd['ms_median'], 3), margin_ms_forward_spread=margin,
               expectation_backward_no_slower_than_forward_met=bwd['ms_median'] <= fwd['ms_median'] + margin,
               agents_only_backward_over_forward=round(bwd0['ms_median'] / fwd0['ms_median'], 3),
               expectation_agents_only_backward_within_2x_forward_met=bwd0['ms_median'] <= 2 * fwd0['ms_median'], rows=[by[k] for k in STEPS])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: f"{by[k]['ms_median']} ({by[k]['ms_min']} - {by[k]['ms_max']})" for k in STEPS}), flush=True)


if __name__ == '__main__':
    main()
