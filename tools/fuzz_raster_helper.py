"""tests/fuzz_raster.py, unchanged, with every launch on the raster stream and the metric stream as its helper (testing build, threshold knob 0:
the fuzzer's 512 cameras per launch are below the product's threshold).  Arguments: those of tests/fuzz_raster.py.
   python tools/fuzz_raster_helper.py --seeds 16 --batch 8 --agents 64 --res 256 --fov 35 [--u8] [--map mixed]"""
import os, runpy, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.chdir(ROOT); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from torchdrivesim_amd import _native as nat, _ops
with nat.testing() as T:
    T.tds_raster_set_helper_min_items(0)
    rs, ms = _ops.reserved_streams(torch.device('cuda:0'))
    plain = _ops.raster_scene
    used = [0, 0]
    def with_helper(*a, **k):
        k.setdefault('helper_stream', ms)
        out = plain(*a, **k)
        used[0] += 1; used[1] += int(_ops.last_helper_workgroups == 96)
        return out
    _ops.raster_scene = with_helper
    sys.argv = ['tests/fuzz_raster.py'] + sys.argv[1:]
    with torch.cuda.stream(rs):
        try:
            runpy.run_path('tests/fuzz_raster.py', run_name='__main__')
        except SystemExit as e:
            print('fuzz_raster exit', e.code)
    torch.cuda.synchronize()
    print(f'helper used in {used[1]} of {used[0]} launches', flush=True)
    _ops.raster_scene = plain
    _ops.map_cache.clear()
    import gc; gc.collect()
    T.tds_raster_set_helper_min_items(4)
