#!/usr/bin/env python3
"""Work counters of the K3 bit-plane kernel on the bench workload (debug flag 128): per wave and image; then the counters of small faces
(tds_raster_get_small_stats: all vertices inside the image, at most TDS_RASTER_SMALL_ROWS rows), per image, overall and per grid chunk.
   python tools/raster_stats.py [B] [RES] [split|fused] [OUT.json]"""
import ctypes, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from torchdrivesim_amd import _native
from torchdrivesim_amd.utils import Resolution
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
RES = int(sys.argv[2]) if len(sys.argv) > 2 else 256
dev = torch.device('cuda', 0)
L = _native.testing_lib()           # the work counters exist only in the testing build
_native._lib = L
sim, actions, _ = bench.build_simulator(B, 64, dev, seed=1234)
for i in range(5):
    sim.step(actions[i % 8])
buf = (ctypes.c_ulonglong * 16)()
sim.render_egocentric(res=Resolution(RES, RES), fov=35.0); torch.cuda.synchronize()
L.tds_raster_get_stats(buf)
small = (ctypes.c_ulonglong * 16)()
L.tds_raster_get_small_stats(small)
SPLIT = len(sys.argv) > 3 and sys.argv[3] == 'split'   # 'split': whatever form the library chooses at this resolution (K3s + K3r below 144 / 208 pixels)
L.tds_raster_set_debug(128 if SPLIT else 128 | 8192)          # default: the fused kernel at every resolution
sim.render_egocentric(res=Resolution(RES, RES), fov=35.0); torch.cuda.synchronize()
L.tds_raster_set_debug(0)
L.tds_raster_get_stats(buf)
names = ['batches', 'faces', 'fill chunks', 'fill windows', 'fill rows', 'edges', 'edge rounds', 'V chunks', 'V windows', 'V rows', 'H chunks',
         'H windows', 'H rows', 'V edges', 'clipped edges', 'faces with rows']
nimg = B * 64
for n, v in zip(names, buf):
    print(f'{n:14s} {v / nimg:10.1f} per image {v / nimg / 4:10.2f} per wave')
L.tds_raster_get_small_stats(small)
s = [int(v) for v in small]
buckets = ['0', '1-8', '9-16', '17-24', '25-32', '33-40', '41-48', '49-64']
import re
ROWS = int(re.search(r'#define TDS_RASTER_SMALL_ROWS (\d+)', open(os.path.join(ROOT, 'include', 'tdship.h')).read()).group(1))   # (of the default build)
report = {'batch': B, 'agents': 64, 'res': RES, 'images': nimg, 'small_rows': ROWS,
          'map_chunks_per_image': s[0] / nimg, 'map_chunks_without_a_face_per_image': s[14] / nimg,
          'map_faces_accepted_per_image': s[1] / nimg, 'map_faces_small_per_image': s[2] / nimg, 'small_share_of_map_faces': s[2] / max(s[1], 1),
          'other_faces_accepted_per_image': s[3] / nimg, 'other_faces_small_per_image': s[4] / nimg,
          'small_faces_per_map_chunk': s[2] / max(s[0], 1), 'small_faces_per_map_chunk_with_a_face': s[2] / max(s[0] - s[14], 1),
          'map_chunks_by_small_faces_share': {b: s[5 + i] / max(s[0], 1) for i, b in enumerate(buckets)},
          'small_faces_in_chunks_that_reach_the_minimum_share': s[13] / max(s[2], 1),
          'batches_per_image': int(buf[0]) / nimg, 'queued_faces_per_image': int(buf[1]) / nimg}
print(json.dumps(report, indent=1))
if len(sys.argv) > 4:
    with open(sys.argv[4], 'w') as f:
        json.dump(report, f, indent=1)
        f.write('\n')
