"""The table behind HELPER_MIN_ITEMS_PER_WG (csrc/tds_raster_plan.h): launch and step times of the 'reserved' loop with an owned
ring at B = 16, 64, 256 and 1024, helper off / on alternating (testing build, threshold knob 0), and the helper's share of the items.
   python tools/helper_cus_timing.py [out.json]"""
import ctypes, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.chdir(ROOT); sys.path.insert(0, ROOT)
import bench
from torchdrivesim_amd import _native as nat, _ops
from torchdrivesim_amd.utils import Resolution
dev = torch.device('cuda:0')
res = Resolution(256, 256)
out = {}
with nat.testing() as T:
    T.tds_raster_set_helper_min_items(0)
    for B in (16, 64, 256, 1024):
        sim, actions, _ = bench.build_simulator(B, 64, dev, seed=1)
        sim.overlap_infractions = 'reserved'
        rs = sim.raster_stream()
        ring = [_ops.owned_image((B, 64, 3, 256, 256), torch.float32, dev) for _ in range(2)]
        rows = {}
        with torch.cuda.stream(rs):
            def step(i):
                sim.step(actions[i % actions.shape[0]])
                sim.render_egocentric(res=res, fov=35.0, out=ring[i % 2])
                sim.compute_collision(); sim.compute_offroad()
            for rep in range(3):
                for helper in (False, True):
                    _ops.use_helper_cus = helper
                    for i in range(6):
                        step(i)
                    torch.cuda.synchronize()
                    _ops.raster_events = []
                    t0 = time.perf_counter()
                    n = 30 if B < 1024 else 12
                    for i in range(n):
                        step(6 + i)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / n * 1e3
                    ms = sum(a.elapsed_time(b) for a, b in _ops.raster_events) / len(_ops.raster_events)
                    _ops.raster_events = None
                    rows.setdefault('on' if helper else 'off', []).append(dict(launch_ms=round(ms, 4), step_ms=round(dt, 4), helper_workgroups=_ops.last_helper_workgroups))
            # the helper's share of the items (counters on: not timed)
            _ops.use_helper_cus = True
            T.tds_raster_set_debug(int(nat.RasterDebug.STATS))
            torch.cuda.synchronize()
            both, h = (ctypes.c_ulonglong * 2)(), (ctypes.c_ulonglong * 1)()
            T.tds_raster_get_prep_stats(both); T.tds_raster_get_helper_stats(h)
            for i in range(4):
                step(i)
            torch.cuda.synchronize()
            T.tds_raster_get_prep_stats(both); T.tds_raster_get_helper_stats(h)
            T.tds_raster_set_debug(0)
            rows['helper_items_of'] = [int(h[0]), int(both[0]) + int(both[1])]
        rows['items_per_main_workgroup'] = round(B * 64 / min(B * 64, 672), 2)
        out[f'B={B}'] = rows
        print(f'B={B}', json.dumps(rows), flush=True)
        del ring, sim
        torch.cuda.empty_cache()
    T.tds_raster_set_helper_min_items(4)
    _ops.use_helper_cus = True
    _ops.map_cache.clear()
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else 'helper_cus_threshold.json', 'w'), indent=1)
