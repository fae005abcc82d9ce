"""Launch times of the semantic masks beside the colour image, on one MI355X: Simulator.render_egocentric_semantic (uint8 masks and packed
bits, the default channels) and render_egocentric (float32 and uint8 RGB) for the same simulator, cameras and run.  bench.py's scene (Town01,
B scenes x A agents, one camera per agent); every launch renders into a caller-owned buffer (out=), HIP events around each of --reps launches
after --warmup, the median and the range printed per (resolution, output).

    python tools/semantic_masks_timing.py [--batch 1024] [--agents 64] [--res 256 128 64] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_launches(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for r in range(reps):
        fn()
        ev[r + 1].record()
    torch.cuda.synchronize()
    return [ev[r].elapsed_time(ev[r + 1]) for r in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--res', type=int, nargs='+', default=[256, 128, 64])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--fov', type=float, default=35.0)
    args = ap.parse_args()
    import bench
    from torchdrivesim_amd.utils import Resolution
    dev = torch.device('cuda', 0)
    sim, _, _ = bench.build_simulator(args.batch, args.agents, dev, seed=0)
    chans = sim.semantic_channels()
    B, A, C = args.batch, args.agents, len(chans)
    rows = []
    for res in args.res:
        r = Resolution(res, res)
        runs = (('rgb_f32', lambda out: sim.render_egocentric(res=r, fov=args.fov, out=out), (B, A, 3, res, res), torch.float32, 'float32'),
                ('rgb_u8', lambda out: sim.render_egocentric(res=r, fov=args.fov, out=out), (B, A, 3, res, res), torch.uint8, 'uint8'),
                ('mask_u8', lambda out: sim.render_egocentric_semantic(res=r, fov=args.fov, out=out), (B, A, C, res, res), torch.bool, None),
                ('mask_bits', lambda out: sim.render_egocentric_semantic(res=r, fov=args.fov, packed=True, out=out),
                 (B, A, C, (res + 31) // 32, res), torch.int32, None))
        for name, fn, shape, dtype, out_dtype in runs:
            if out_dtype is not None:
                sim.renderer.cfg.out_dtype = out_dtype
            out = torch.empty(shape, dtype=dtype, device=dev)
            ms = sorted(time_launches(lambda: fn(out), args.reps, args.warmup))
            row = dict(res=res, output=name, channels=C if name.startswith('mask') else 3, bytes=out.numel() * out.element_size(),
                       ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3), ms_max=round(ms[-1], 3))
            row['tb_per_s'] = round(row['bytes'] / (row['ms_median'] * 1e-3) / 1e12, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out
            torch.cuda.empty_cache()
        sim.renderer.cfg.out_dtype = 'float32'
    print(json.dumps(dict(batch=B, agents=A, channels=chans, device=torch.cuda.get_device_name(dev))))


if __name__ == '__main__':
    main()
