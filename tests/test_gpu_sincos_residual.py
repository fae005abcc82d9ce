"""The product, with the device's sin / cos, against the reference's numbers, whose sin / cos come from torch on a CPU: counted on 512 cameras.

Three statements, each asserted:
  * torch.sin / torch.cos on the device is within k ulp of torch on the CPU (a pin of the environment, recorded in profiles/sincos_residual.json);
  * fed the device's [sin, cos], the product equals the oracle bit for bit (images float32 and uint8, collision values, off-road values) -- so whatever
    separates the product from the reference's numbers is a statement about [sin, cos] alone;
  * that residual (pixels, `collision > 0` flags for both metrics, `offroad > 0` flags) does not exceed what the ORACLE shows when every [sin, cos] value
    it is fed is moved k ulp at random -- a bound taken from the reference side only.  Where that stand-in moves nothing, this is exact equality.
The workload, the stand-ins and the counting live in test_sincos_residual_model.py, which checks them on the CPU.
Set TDS_SINCOS_RESIDUAL_OUT=<file> to have the measured record written as JSON (that is how profiles/sincos_residual.json was made).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_sincos_residual_model import FLAG_KINDS, OFFROAD_THRESHOLD, cpu_sc, moved_ulp, oracle_outputs, residual, subset, ulp_distance, workload

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PROFILE = os.path.join(ROOT, 'profiles', 'sincos_residual.json')
IMAGE_SEEDS, FLAG_SEEDS = 3, 32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_sc(psi):
    from torchdrivesim_amd import _ops
    return _ops.heading_sc(dev(np.ascontiguousarray(psi, dtype=np.float32))).cpu().numpy()


def versions():
    return dict(torch=torch.__version__, hip=torch.version.hip, device=torch.cuda.get_device_name(0))


def record(section, figures):
    line = json.dumps({section: figures}, sort_keys=True)
    print('\nsincos_residual ' + line)
    path = os.environ.get('TDS_SINCOS_RESIDUAL_OUT')
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.update({section: figures, 'versions': versions()})
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')


def ulp_figures(psi):
    psi = np.ascontiguousarray(psi, dtype=np.float32).reshape(-1)
    d = ulp_distance(device_sc(psi), cpu_sc(psi)).reshape(-1)
    hist = np.bincount(np.minimum(d, 8).astype(np.int64), minlength=9)
    return dict(values=int(d.size), differ_share=float((d > 0).mean()), max_ulp=int(d.max()), histogram_ulp_0_to_8_or_more=[int(x) for x in hist])


def stand_in_bounds(oracle, w, base, base_sc, k, buf=None):
    """The oracle fed `base_sc` with every value moved k ulp at random against the oracle fed `base_sc`: images for IMAGE_SEEDS seeds, flags for FLAG_SEEDS.
    Returns the largest counts and every seed's counts."""
    px, flags = [], {kind: [] for kind in FLAG_KINDS}
    for seed in range(FLAG_SEEDS):
        r = residual(base, oracle_outputs(oracle, w, moved_ulp(base_sc, k, seed), images=seed < IMAGE_SEEDS, out=buf), images=seed < IMAGE_SEEDS)
        if seed < IMAGE_SEEDS:
            px.append(dict(pixels=r['pixels'], cameras=r['cameras'], most_in_one_camera=r['most_in_one_camera']))
        for kind in FLAG_KINDS:
            flags[kind].append(len(r[kind]))
    return dict(k_ulp=k, pixels=max(p['pixels'] for p in px), pixel_runs=px, **{kind: max(v) for kind, v in flags.items()},
                flag_runs=flags)


def describe(r, a_name, b_name):
    lines = [f"  scene {s} camera {a}: {n} pixels" for s, a, n in r.get('camera_list', [])]
    for kind in FLAG_KINDS:
        lines += [f'  {kind} flag of scene {s} agent {a}: {x!r} {a_name}, {y!r} {b_name}' for s, a, x, y in r[kind]]
    return '\n'.join(lines)


def check_inside(r, bound, what):
    text = describe(r, 'from the product', 'from the oracle fed torch-CPU [sin, cos]')
    if text:
        print(f'{what}: what differs\n{text}')
    assert r['pixels'] <= bound['pixels'], f"{what}: {r['pixels']} pixels differ, the {bound['k_ulp']}-ulp stand-ins reach {bound['pixels']}\n{text}"
    for kind in FLAG_KINDS:
        assert len(r[kind]) <= bound[kind], f"{what}: {len(r[kind])} {kind} flags differ, the {bound['k_ulp']}-ulp stand-ins reach {bound[kind]}\n{text}"


def counts(r):
    return dict(pixels=r['pixels'], total_pixels=r['total_pixels'], cameras=r['cameras'], most_in_one_camera=r['most_in_one_camera'],
                **{kind: len(r[kind]) for kind in FLAG_KINDS})


@pytest.fixture(scope='module')
def k_ulp():
    """the largest ulp distance of device against CPU sin / cos over the workload's own headings (at least 1), with the figures it came from"""
    w = workload()
    g2, g13 = load_golden('g2_boxes.npz'), load_golden('g13_discs_n.npz')
    golden = np.concatenate([g2[f'{t}_box{i}'][:, 4] for t in ('cur', 'rnd0', 'rnd400') for i in (1, 2)] + [g13['box1'][:, 4], g13['box2'][:, 4]])
    golden = golden[np.isfinite(golden)]
    fig = dict(workload=ulp_figures(w['state'][..., 2]), sweep=ulp_figures(np.linspace(-np.pi, np.pi, 1 << 20, dtype=np.float64).astype(np.float32)),
               golden_headings=ulp_figures(golden))
    return max(1, fig['workload']['max_ulp']), fig


def test_device_sincos_is_within_the_recorded_ulp_of_the_cpu(k_ulp):
    """torch and the ROCm math library, not this project's code: a pin of the environment.  A toolchain whose sin / cos move twice as far from the CPU's as
    the recorded one is noticed here, before it shows as pixels."""
    k, fig = k_ulp
    record('ulp', dict(k=k, **fig))
    recorded = json.load(open(PROFILE))['ulp']['k']
    assert k <= 2 * recorded, f'device sin / cos are up to {k} ulp from torch-CPU on the workload, {recorded} recorded in profiles/sincos_residual.json ' \
                              f'(torch {torch.__version__}, HIP {torch.version.hip}): {fig}'
    assert fig['sweep']['max_ulp'] <= 2 * max(recorded, json.load(open(PROFILE))['ulp']['sweep']['max_ulp']), fig['sweep']


def test_kernels_equal_the_oracle_and_the_residual_is_the_sincos_alone(oracle, k_ulp):
    from torchdrivesim_amd import _ops as ops
    from test_gpu_parity import actor_keys, make_map
    k, _ = k_ulp
    w = workload()
    st, sz, pr, res = w['state'], w['size'], w['present'], w['res']
    B, A = pr.shape
    sc_cpu, sc_dev = cpu_sc(st[..., 2]), device_sc(st[..., 2])
    r_cpu = oracle_outputs(oracle, w, sc_cpu)
    r_dev = oracle_outputs(oracle, w, sc_dev)
    assert (r_cpu['img'] > 0).mean() > 0.05
    # the product on the device's [sin, cos]: the scene rasteriser, the scene collision kernel, the off-road kernel
    smap = make_map(ops, w['verts'], w['faces'], w['vert_category'], w['categories'])
    sd, scd = dev(st), dev(sc_dev)
    assert np.array_equal(ops.heading_sc(sd[..., 2]).cpu().numpy(), sc_dev)
    tmpl, keys, mask, cam_xy = dev(oracle.actor_template(sz)), actor_keys(smap, B, A), dev(w['mask']), dev(st[..., :2].copy())
    p8 = ops.raster_scene(smap, sd, scd, tmpl, keys, mask, cam_xy, scd, w['fov'], res, torch.uint8).cpu().numpy()
    bad = p8.astype(np.float32) != r_dev['img']
    assert not bad.any(), f'uint8: {bad.sum()} values differ from the oracle fed the same [sin, cos]'
    del p8, bad
    p = dict(img=ops.raster_scene(smap, sd, scd, tmpl, keys, mask, cam_xy, scd, w['fov'], res, torch.float32).cpu().numpy())
    bad = p['img'] != r_dev['img']
    assert not bad.any(), f'float32: {bad.sum()} values differ from the oracle fed the same [sin, cos]'
    del bad
    boxes = dev(np.concatenate([st[..., :2], sz, st[..., 2:3]], -1))
    for metric in ('iou', 'discs'):
        p[metric] = ops.collision(boxes, dev(pr), metric=metric, sc=scd).cpu().numpy()
    geo = make_map(ops, w['verts'], w['faces'], None, None, render=False)
    p['offroad'] = ops.offroad_forward(geo, sd, dev(sz), scd, dev(pr), OFFROAD_THRESHOLD).cpu().numpy()
    for kind in FLAG_KINDS:
        assert np.array_equal(p[kind], r_dev[kind]), f'{kind}: the kernel differs from the oracle fed the same [sin, cos]'
    # the residual: the product against the reference's numbers (the oracle fed torch-CPU [sin, cos]) ...
    r = residual(p, r_cpu)
    del p, r_dev
    # ... inside what the oracle itself shows when every [sin, cos] value moves k ulp
    bound = stand_in_bounds(oracle, w, r_cpu, sc_cpu, k, buf=np.empty_like(r_cpu['img']))
    record('kernels_512_cameras', dict(sc_differ_share=float((sc_dev != sc_cpu).mean()), device=counts(r), stand_in=bound,
                                        flags_listed={kind: r[kind] for kind in FLAG_KINDS}))
    check_inside(r, bound, '512 cameras through the kernels')
    assert r['most_in_one_camera'] < 0.01 * res * res


def test_simulator_residual_on_64_cameras(oracle, k_ulp):
    """the same comparison once through the public surface: Simulator.render_egocentric / compute_collision / compute_offroad on the first two scenes"""
    from test_gpu_simulator import make_sim, town_mesh
    from torchdrivesim_amd.simulator import CollisionMetric
    from torchdrivesim_amd.utils import Resolution
    k, _ = k_ulp
    w = subset(workload(), 2)
    st, sz, pr = w['state'], w['size'], w['present']
    sc_cpu = cpu_sc(st[..., 2])
    r_cpu = oracle_outputs(oracle, w, sc_cpu)
    road, _ = town_mesh(2)
    sim = make_sim(st, sz, pr, road)
    assert sim.cfg.offroad_threshold == OFFROAD_THRESHOLD
    p = dict(img=sim.render_egocentric(res=Resolution(w['res'], w['res']), fov=w['fov']).cpu().numpy(), offroad=sim.compute_offroad().cpu().numpy())
    for metric in ('iou', 'discs'):
        sim.cfg.collision_metric = CollisionMetric(metric)
        p[metric] = sim.compute_collision().cpu().numpy()
    r_dev = oracle_outputs(oracle, w, device_sc(st[..., 2]))
    for kind in ('img',) + FLAG_KINDS:
        assert np.array_equal(p[kind], r_dev[kind]), f'{kind}: the simulator differs from the oracle fed the same [sin, cos]'
    r = residual(p, r_cpu)
    bound = stand_in_bounds(oracle, w, r_cpu, sc_cpu, k)
    record('simulator_64_cameras', dict(device=counts(r), stand_in=bound, flags_listed={kind: r[kind] for kind in FLAG_KINDS}))
    check_inside(r, bound, '64 cameras through the Simulator')
