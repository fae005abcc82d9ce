"""What another sin / cos does to the outputs, measured on the oracle alone (no GPU).

Every kernel equals the oracle bit for bit when both are fed the same [sin psi, cos psi], and the oracle equals the reference's recorded outputs.  The
remaining link is the [sin, cos] itself: the reference takes it from torch on the CPU, the product from torch on the device.  This module builds one
fixed workload (512 egocentric cameras on Town01), feeds the oracle [sin, cos] arrays from different sources and counts what changes: pixels,
`collision > 0` flags (iou and discs) and `offroad > 0` flags.  tests/test_gpu_sincos_residual.py imports the workload and the counting from here and
puts the device's own [sin, cos] through the same comparison, bounded by the stand-ins computed here.
"""
import numpy as np
import torch

from conftest import load_golden

SEED, SCENES, AGENTS, RES, FOV = 20260, 16, 32, 256, 35.0
OFFROAD_THRESHOLD = 0.5


def workload(scenes=SCENES, agents=AGENTS, seed=SEED):
    """`scenes` x `agents` random poses around Town01 road vertices (as test_k3_random_town01_256_bit_exact places them), 90 % of the agents present, every
    present agent a camera that sees the present agents.  Lengths exceed widths, so the discs metric uses the heading's own [sin, cos]."""
    t = load_golden('town01_mesh.npz')
    verts, faces, vcat, cats = t['verts'], t['faces'], t['vert_category'], [str(c) for c in t['categories']]
    gen = np.random.default_rng(seed)
    B, A = scenes, agents
    road = verts[vcat == cats.index('road')]
    anchor = road[gen.integers(0, len(road), (B, 1))]
    xy = anchor + gen.uniform(-25, 25, (B, A, 2))
    state = np.concatenate([xy, gen.uniform(-np.pi, np.pi, (B, A, 1)), gen.uniform(0, 10, (B, A, 1))], -1).astype(np.float32)
    size = np.concatenate([gen.uniform(4, 5, (B, A, 1)), gen.uniform(1.8, 2.2, (B, A, 1))], -1).astype(np.float32)
    present = gen.uniform(size=(B, A)) < 0.9
    mask = np.ascontiguousarray(np.broadcast_to(present[:, None, :], (B, A, A)))
    return dict(state=state, size=size, present=present, mask=mask, verts=verts, faces=faces, vert_category=vcat, categories=cats, res=RES, fov=FOV)


def subset(w, scenes):
    """the first `scenes` scenes of a workload"""
    return {k: (v[:scenes] if k in ('state', 'size', 'present', 'mask') else v) for k, v in w.items()}


def cpu_sc(psi):
    """[sin, cos] as the reference computes them: torch.sin / torch.cos on CPU tensors"""
    p = torch.from_numpy(np.ascontiguousarray(psi, dtype=np.float32))
    return torch.stack([torch.sin(p), torch.cos(p)], -1).numpy()


def moved_ulp(sc, k, seed):
    """every value moved k float32 ulp, up or down at random"""
    up = np.random.default_rng(seed).integers(0, 2, sc.shape).astype(bool)
    toward = np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    out = sc.astype(np.float32)
    for _ in range(k):
        out = np.nextafter(out, toward)
    return out


def ulp_distance(a, b):
    """distance of two float32 arrays in representable values (0: same bits, or +0 against -0)"""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def oracle_outputs(orc, w, sc, images=True, out=None):
    """The oracle on workload `w` with cameras AND agents turned by `sc` (B x A x 2): images (B x A x 3 x H x W, or None), the scene collision values for
    both metrics and the off-road values."""
    sc = np.ascontiguousarray(sc, dtype=np.float32)
    st, sz, pr = w['state'], w['size'], w['present']
    img = None
    if images:
        static = orc.static_mesh_arrays(w['verts'], w['faces'], w['vert_category'], w['categories'])
        img = orc.render_scenes(st, sz, w['mask'], st[..., :2].copy(), sc, *static, w['fov'], w['res'], agent_sc=sc, out=out)
    boxes = np.concatenate([st[..., :2], sz, st[..., 2:3]], -1)
    return dict(img=img, iou=orc.collision(boxes, pr, metric='iou', sc=sc), discs=orc.collision(boxes, pr, metric='discs', sc=sc),
                offroad=orc.offroad(st, sz, w['verts'], w['faces'], OFFROAD_THRESHOLD, present=pr, sc=sc))


FLAG_KINDS = ('iou', 'discs', 'offroad')


def residual(a, b, images=True):
    """What differs between two sets of outputs: pixels (a pixel counts once if any channel differs), the cameras they are in, the most in one camera, and the
    agents whose `value > 0` flag differs for each kind, as (scene, agent, value in a, value in b)."""
    r = {}
    if images:
        px = (a['img'] != b['img']).any(axis=2)                              # B x A x H x W
        per_cam = px.reshape(px.shape[0] * px.shape[1], -1).sum(1)
        r.update(pixels=int(per_cam.sum()), total_pixels=int(px.size), cameras=int((per_cam > 0).sum()), most_in_one_camera=int(per_cam.max()),
                 camera_list=[(int(i // px.shape[1]), int(i % px.shape[1]), int(per_cam[i])) for i in np.nonzero(per_cam)[0]])
    for kind in FLAG_KINDS:
        x, y = np.asarray(a[kind]), np.asarray(b[kind])
        r[kind] = [(int(s), int(g), float(x[s, g]), float(y[s, g])) for s, g in zip(*np.nonzero((x > 0) != (y > 0)))]
    return r


def row(name, sc, base_sc, r):
    px = f"{r['pixels']:6d} {r['cameras']:4d} {r['most_in_one_camera']:4d}" if 'pixels' in r else f"{'-':>6} {'-':>4} {'-':>4}"
    return (f"{name:34s} sc differ {100.0 * (sc != base_sc).mean():5.1f} %  pixels / cameras / most {px}  "
            f"flags iou {len(r['iou'])} discs {len(r['discs'])} offroad {len(r['offroad'])}")


def test_another_sincos_moves_a_handful_of_pixels_and_no_disc_or_offroad_flag(oracle):
    """The counting itself, on the CPU: identical [sin, cos] give identical outputs; numpy's float32 sin / cos, float64 sin / cos rounded, and every value moved
    one or two ulp change fewer than 1e-4 of the pixels (measured here: at most a few per million), while [sin, cos] computed in float16 -- a genuinely wrong
    input -- exceed that share, so the comparison looks at the right things; no 1-ulp stand-in moves a disc or an off-road flag.  Prints the table."""
    w = workload()
    psi = w['state'][..., 2]
    base_sc = cpu_sc(psi)
    base = oracle_outputs(oracle, w, base_sc)
    assert (base['img'] > 0).mean() > 0.05 and w['present'].mean() > 0.8
    for kind in FLAG_KINDS:                                                      # the workload has agents on both sides of every flag
        assert 0.02 < (base[kind] > 0).mean() < 0.98, kind
    buf = np.empty_like(base['img'])
    again = oracle_outputs(oracle, w, base_sc.copy(), out=buf)
    r = residual(base, again)
    assert r['pixels'] == 0 and not any(r[k] for k in FLAG_KINDS)
    for k in FLAG_KINDS:
        assert np.array_equal(base[k], again[k])
    print()
    print(row('torch-CPU again', base_sc, base_sc, r))
    p64 = psi.astype(np.float64)
    stand_ins = [('float64 sin / cos, rounded', np.stack([np.sin(p64), np.cos(p64)], -1).astype(np.float32)),
                 ('numpy float32', np.stack([np.sin(psi), np.cos(psi)], -1))]
    stand_ins += [(f'every value moved {k} ulp, seed {s}', moved_ulp(base_sc, k, s)) for k in (1, 2) for s in range(3)]
    for name, sc in stand_ins:
        assert ulp_distance(sc, base_sc).max() <= 2, name
        r = residual(base, oracle_outputs(oracle, w, sc, out=buf))
        print(row(name, sc, base_sc, r))
        for kind in FLAG_KINDS:
            for s, a, x, y in r[kind]:
                print(f'    {kind} flag of scene {s} agent {a}: {x!r} with torch-CPU [sin, cos], {y!r} with this one')
        assert r['pixels'] < 1e-4 * r['total_pixels'], f"{name}: {r['pixels']} of {r['total_pixels']} pixels differ"
        assert r['most_in_one_camera'] < 0.01 * RES * RES, name                 # never a whole camera
        if 'moved 1 ulp' in name:
            assert not r['discs'] and not r['offroad'], f'{name}: {r["discs"]} {r["offroad"]}'
    # the control: [sin, cos] computed in float16 and widened are wrong by 2^-11, and the count says so
    w64 = subset(w, 2)
    h = torch.from_numpy(psi[:2].copy()).to(torch.float16)
    sc16 = torch.stack([torch.sin(h.float()).to(torch.float16), torch.cos(h.float()).to(torch.float16)], -1).float().numpy()
    b64 = dict(img=base['img'][:2], **{k: base[k][:2] for k in FLAG_KINDS})
    r = residual(b64, oracle_outputs(oracle, w64, sc16))
    print(row('float16 (64 cameras, must be caught)', sc16, base_sc[:2], r))
    assert r['pixels'] > 1e-4 * r['total_pixels'], 'float16 [sin, cos] passed the bound the stand-ins are held to: the comparison is blind'
