#!/usr/bin/env python3
"""
The reference's examples/initialize_simulation.py with method='heuristic' on this framework: put agents on the lanes of the Town01 package
shipped under tests/golden/ (mesh + lane map), build a Simulator from them and render the world view.  The image is written as a binary PPM
with numpy alone.

    python examples/initialize_simulation.py [--agents 64] [--seed 0] [--res 1024] [--fov 400] [--out initialization.ppm]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the Town01 mesh, shared with the benchmark)
from torchdrivesim_amd import lanelet2  # noqa: E402
from torchdrivesim_amd.behavior import heuristic_initialize  # noqa: E402
from torchdrivesim_amd.kinematic import KinematicBicycle  # noqa: E402
from torchdrivesim_amd.mesh import BirdviewMesh  # noqa: E402
from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config  # noqa: E402
from torchdrivesim_amd.simulator import Simulator, TorchDriveConfig  # noqa: E402
from torchdrivesim_amd.utils import Resolution  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--res', type=int, default=1024)
    ap.add_argument('--fov', type=float, default=400.0)
    ap.add_argument('--out', default='initialization.ppm')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lanes = lanelet2.load_lanelet_map(os.path.join(ROOT, 'tests', 'golden', 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    attributes, states = heuristic_initialize(lanes, args.agents, seed=args.seed, device=dev)          # (1, A, 3), (1, A, 4), on the device

    verts, faces, vcat, cats = bench.load_town01()
    road = BirdviewMesh(verts=torch.from_numpy(verts)[None], faces=torch.from_numpy(faces.astype(np.int64))[None], categories=cats, colors={}, zs={},
                        vert_category=torch.from_numpy(vcat.astype(np.int64))[None]).to(dev)
    model = KinematicBicycle()
    model.set_params(lr=attributes[..., 2].contiguous())
    model.set_state(states)
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    res = Resolution(args.res, args.res)
    sim = Simulator(road, model, attributes[..., :2].contiguous(), torch.ones_like(states[..., 0], dtype=torch.bool), cfg,
                    renderer=renderer_from_config(cfg.renderer, res=res, fov=args.fov), lanelet_map=[lanes])
    centre = sim.get_world_center().to(dev).reshape(1, 1, 2)
    image = sim.render(camera_xy=centre, camera_psi=torch.full((1, 1, 1), float(np.pi / 2), device=dev), res=res, fov=args.fov)
    rgb = image[0, 0].permute(1, 2, 0).cpu().numpy().astype(np.uint8)
    with open(args.out, 'wb') as f:
        f.write(b'P6 %d %d 255\n' % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb).tobytes())
    print(f'{args.agents} agents on Town01 (seed {args.seed}): collisions {int((sim.compute_collision() > 0).sum())}, '
          f'wrong way {int((sim.compute_wrong_way() > 0).sum())}; wrote {args.out}')


if __name__ == '__main__':
    main()
