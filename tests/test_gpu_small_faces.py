"""The persistent bit-plane kernel paints SMALL faces -- all three vertices inside the image, at most TDS_RASTER_SMALL_ROWS rows -- on the lane
that scanned them (raster.hip: drain_bits, process_small_bits<ROWS>) whenever enough lanes of a scan step hold one.  Every image here equals the
oracle's byte for byte and equals the render with the path switched off (small_faces=False: TDS_RASTER_NO_SMALL_FACES), in the testing build and in
the product; the testing build's counter shows that faces took the path, so that no test passes vacuously.  256 x 256 is the smallest side at which
the persistent five-key instantiation is what runs; at 192 x 192 the plan has no such launch and the path is not taken."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_parity import COLORS, LEVELS, LEVEL_TABLE, actor_keys, dev, make_map, oracle_static, pack, sc_np

pytestmark = pytest.mark.gpu
FOV, RES, ROWS = 35.0, 256, 7
FOVS = (35.0, 70.0)              # the benchmark's, and one at which faces are half the size and a scan step mixes more of them
CATS = ['road', 'left_lane', 'right_lane']


@pytest.fixture(scope='module')
def ops():
    from torchdrivesim_amd import _ops
    return _ops


def project(verts, cam_xy, psi, res, fov):
    """integer pixel coordinates as the kernel and the oracle compute them (float32)"""
    f32 = np.float32
    s, c = f32(np.sin(f32(psi))), f32(np.cos(f32(psi)))
    x, y = verts[:, 0].astype(f32) - f32(cam_xy[0]), verts[:, 1].astype(f32) - f32(cam_xy[1])
    scale = f32(2.0) / f32(fov)
    rx, ry = (-(c * x + s * y)) * scale, (-((-s) * x + c * y)) * scale
    rx, ry = rx * f32(res) / f32(2) + f32(res) / f32(2), ry * f32(res) / f32(2) + f32(res) / f32(2)
    return np.trunc(rx).astype(np.int64), np.trunc(ry).astype(np.int64)


def pixel_to_world(p, cam_xy, psi, fov, res=256):
    """the world point that `project` sends to the (fractional) pixel p"""
    u, v = -(p[0] - res / 2) * fov / res, -(p[1] - res / 2) * fov / res
    c, s = np.cos(psi), np.sin(psi)
    return cam_xy[0] + c * u - s * v, cam_xy[1] + s * u + c * v


def synthetic_map():
    """about 5 800 faces over 64 m x 64 m around the origin, far beyond every view below: a lattice of sliver quads 3 .. 7 pixels long and one
    or two wide in every direction (0.137 m per pixel), tiny faces of one and two rows, faces with a repeated vertex, faces whose height steps
    through 0.7 .. 1.1 m (exactly ROWS - 1 and ROWS rows of pixels among them), and one face that reaches 5 km out of the view (outside the
    packed coordinate range); the lattice crosses every border and corner of every view"""
    gen = np.random.default_rng(5)
    px = FOV / RES
    verts, faces, cat = [], [], []

    def tri(a, b, c, k):
        n = len(verts)
        verts.extend([a, b, c]); faces.append((n, n + 1, n + 2)); cat.append(k)

    for gx in np.arange(-32.0, 32.0, 1.1):
        for gy in np.arange(-32.0, 32.0, 1.1):
            o = np.array([gx, gy]) + gen.uniform(-0.2, 0.2, 2)
            th = gen.uniform(0, 2 * np.pi)
            u, v = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
            kind = gen.integers(0, 8)
            k = 1 + int(gen.integers(0, 2))
            if kind < 5:                                       # a sliver quad, as a lane marking's
                ln, wd = gen.uniform(3, 7) * px, gen.uniform(0.8, 2.2) * px
                a, b, c, d = o, o + ln * u, o + ln * u + wd * v, o + wd * v
                tri(a, b, c, k); tri(a, c, d, k)
            elif kind == 5:                                    # one or two rows
                tri(o, o + gen.uniform(0.3, 1.5) * px * u, o + gen.uniform(0.3, 1.5) * px * v, k)
            elif kind == 6:                                    # a repeated vertex: a line
                b = o + gen.uniform(1, 7) * px * u
                tri(o, b, b, k) if gen.integers(0, 2) else tri(o, o, b, k)
            else:                                              # heights around the limit of the path
                h = 0.7 + 0.4 * gen.uniform()
                tri(o, o + np.array([gen.uniform(-0.5, 0.5), h]), o + np.array([gen.uniform(0.1, 0.6), gen.uniform(0, h)]), k)
    for i, h in enumerate(np.arange(0.70, 1.10, 0.004)):      # camera 0 looks along x: these heights are rows
        o = np.array([-6.0 + 0.12 * i, 3.0])
        tri(o, o + np.array([0.1, h]), o + np.array([0.25, 0.5 * h]), 2)
    tri(np.array([0.5, 0.5]), np.array([5000.0, 3.0]), np.array([5000.0, -4.0]), 0)
    # a sliver across every corner and the middle of every side of every view below, at both fields of view
    cam_xy, psi = cameras()
    for fov in FOVS:
        for (cx, cy), th in zip(cam_xy[0], psi[0]):
            for qx, qy in ((0, 0), (RES, 0), (0, RES), (RES, RES), (RES // 2, 0), (RES // 2, RES), (0, RES // 2), (RES, RES // 2)):
                w = pixel_to_world((qx - 2.5, qy - 1.5), (cx, cy), th, fov), pixel_to_world((qx + 3.5, qy - 0.5), (cx, cy), th, fov), \
                    pixel_to_world((qx + 0.5, qy + 2.5), (cx, cy), th, fov)
                tri(np.array(w[0]), np.array(w[1]), np.array(w[2]), 2)
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int32)
    vcat = np.zeros(len(verts), np.int64)
    vcat[faces[:, 0]] = cat; vcat[faces[:, 1]] = cat; vcat[faces[:, 2]] = cat
    return verts, faces, vcat


def cameras():
    gen = np.random.default_rng(6)
    psi = np.concatenate([[0.0, np.pi / 4, np.pi / 2], gen.uniform(-np.pi, np.pi, 5)]).astype(np.float32)
    xy = np.concatenate([[[0.0, 0.0]], gen.uniform(-8, 8, (7, 2))]).astype(np.float32)
    return xy[None], psi[None]                                # one scene x 8 cameras


def scene(oracle, B, Nc, gen):
    N = 2
    state = np.concatenate([gen.uniform(-5, 5, (B, N, 2)), gen.uniform(-np.pi, np.pi, (B, N, 1)), np.zeros((B, N, 1))], -1).astype(np.float32)
    size = np.tile(np.array([4.5, 2.0], np.float32), (B, N, 1))
    mask = np.ones((B, Nc, N), bool)
    return state, size, mask


def small_stats(T):
    buf = (ctypes.c_ulonglong * 16)()
    assert T.tds_raster_get_small_stats(buf) == 0
    return [int(v) for v in buf]


def render(ops, oracle, smap, state, size, mask, cam_xy, psi, res, fov=FOV, out_dtype=torch.float32, **kw):
    sd = dev(state)
    return ops.raster_scene(smap, sd, ops.heading_sc(sd[..., 2]), dev(oracle.actor_template(size)), actor_keys(smap, *state.shape[:2]), dev(mask),
                            dev(cam_xy), ops.heading_sc(dev(psi)), fov, res, out_dtype, **kw)


def reference(ops, oracle, static, state, size, mask, cam_xy, psi, res, fov=FOV):
    sv, sa, sf = static
    cam_sc = sc_np(ops.heading_sc(dev(psi)))
    return oracle.render_scenes(state, size, mask, cam_xy, cam_sc, sv, sa, sf, fov, res, agent_sc=sc_np(ops.heading_sc(dev(state[..., 2]))))


def test_the_synthetic_map_holds_the_cases_it_claims():
    verts, faces, _ = synthetic_map()
    cam_xy, psi = cameras()
    X, Y = project(verts, cam_xy[0, 0], psi[0, 0], RES, FOV)
    X, Y = X[faces], Y[faces]
    inside = ((X >= 0) & (X < RES) & (Y >= 0) & (Y < RES)).all(1)
    h = Y.max(1) - Y.min(1)
    for want in (0, 1, ROWS - 1, ROWS):                        # one row, two rows, the last height the path takes, the first it does not
        assert (inside & (h == want)).sum() >= 5, want
    assert 2000 < len(faces) < 12000
    assert np.abs(X).max() >= 32768                          # the face outside the packed range
    assert (faces[:, 1] == faces[:, 2]).sum() + (faces[:, 0] == faces[:, 1]).sum() == 0     # (repeated vertices are repeated positions, not indices)
    assert ((verts[faces[:, 0]] == verts[faces[:, 1]]).all(1) | (verts[faces[:, 1]] == verts[faces[:, 2]]).all(1)).sum() >= 100
    # every view, at both fields of view: slivers of at most ROWS + 1 rows across each of the four sides and over each of the four corners
    for fov in FOVS:
        for k in range(cam_xy.shape[1]):
            X, Y = project(verts, cam_xy[0, k], psi[0, k], RES, fov)
            X, Y = X[faces], Y[faces]
            low = (Y.max(1) - Y.min(1) <= ROWS) & (X.max(1) - X.min(1) <= 2 * ROWS)
            xl, xr = (X.min(1) < 0) & (X.max(1) >= 0), (X.min(1) < RES) & (X.max(1) >= RES)
            yt, yb = (Y.min(1) < 0) & (Y.max(1) >= 0), (Y.min(1) < RES) & (Y.max(1) >= RES)
            for name, sel in (('left', xl), ('right', xr), ('top', yt), ('bottom', yb), ('top-left', xl & yt), ('top-right', xr & yt),
                              ('bottom-left', xl & yb), ('bottom-right', xr & yb)):
                assert (sel & low).sum() >= 1, (fov, k, name)


@pytest.mark.parametrize('fov', FOVS)
@pytest.mark.parametrize('mode', ['float32', 'uint8', 'slices'])
def test_synthetic_slivers_equal_the_oracle_on_and_off_the_path(ops, oracle, mode, fov):
    from torchdrivesim_amd import _native as nat
    verts, faces, vcat = synthetic_map()
    cam_xy, psi = cameras()
    state, size, mask = scene(oracle, 1, 8, np.random.default_rng(7))
    ref = reference(ops, oracle, oracle_static(oracle, verts, faces, vcat, CATS), state, size, mask, cam_xy, psi, RES, fov)
    kw = dict(out_dtype=torch.uint8) if mode == 'uint8' else (dict(index_slices=True) if mode == 'slices' else {})
    kw['fov'] = fov
    image = lambda r: (r[0] if isinstance(r, tuple) else r).cpu().numpy()
    with nat.testing() as T:
        smap = make_map(ops, verts, faces, vcat, CATS)
        try:
            T.tds_raster_set_debug(int(nat.RasterDebug.STATS))
            small_stats(T)
            on = image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, **kw))
            torch.cuda.synchronize()
            s_on = small_stats(T)
            off = image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, small_faces=False, **kw))
            torch.cuda.synchronize()
            s_off = small_stats(T)
        finally:
            T.tds_raster_set_debug(0)
        del smap
    print(f'{mode} fov {fov}: faces painted on their lane {s_on[15]} of {s_on[1] + s_on[3]} accepted ({s_on[2] + s_on[4]} small); path off: {s_off[15]}')
    assert s_on[15] > 0 and s_off[15] == 0
    assert s_on[1] == s_off[1] and s_on[2] == s_off[2]
    assert np.array_equal(on, ref.astype(on.dtype)), int((on != ref).any((2, 3, 4)).sum())
    assert np.array_equal(off, on)
    # the product library, with the path and, through the module switch of _ops, without it
    smap = make_map(ops, verts, faces, vcat, CATS)
    assert np.array_equal(image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, **kw)), on)
    ops.use_small_faces = False
    try:
        assert np.array_equal(image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, **kw)), on)
    finally:
        ops.use_small_faces = True


def test_town01_views_into_an_owned_buffer(ops, oracle):
    """2 scenes x 4 cameras of the benchmark's agent recipe on Town01, rendered twice into one owned buffer so that the second launch skips the
    background lines it need not rewrite; more than half of the accepted faces are painted on the lane that scanned them (the census of
    tools/face_size_census.py: 69 % of the faces in view are small, 94 % of those sit in scan steps with 25 or more of them)"""
    import bench
    from torchdrivesim_amd import _native as nat
    t = load_golden('town01_mesh.npz')
    verts, faces, vcat, cats = t['verts'], t['faces'], t['vert_category'], [str(c) for c in t['categories']]
    st = bench.synth_agents(2, 4, verts[vcat == cats.index('road')], 1234)[0]
    cam_xy, psi = st[..., :2].copy(), st[..., 2].copy()
    state, size, mask = scene(oracle, 2, 4, np.random.default_rng(8))
    state[..., :2] += cam_xy[:, :1]
    ref = reference(ops, oracle, oracle_static(oracle, verts, faces, vcat, cats), state, size, mask, cam_xy, psi, RES)
    cat = np.asarray(vcat)[faces[:, 0]]
    with nat.testing() as T:
        # the grid cells of HipRenderer.make_static_map at this field of view (0.65 fov), as in the benchmark
        smap = ops.StaticMap(np.asarray(verts, np.float32), np.asarray(faces, np.int32), np.array([LEVELS[cats[c]] for c in cat], np.float32),
                             np.array([pack(COLORS[cats[c]]) for c in cat], np.uint32), LEVEL_TABLE, device='cuda:0', cell_size=0.65 * FOV)
        out = ops.owned_image((2, 4, 3, RES, RES), torch.float32, 'cuda:0')
        try:
            render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, out=out)
            first = out.cpu().numpy()
            T.tds_raster_set_debug(int(nat.RasterDebug.STATS))
            small_stats(T)
            render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, out=out)
            torch.cuda.synchronize()
            s = small_stats(T)
        finally:
            T.tds_raster_set_debug(0)
        second = out.cpu().numpy()
        rec = ops._owned_buffers[out.data_ptr()]['record']
        del smap, out
    share = s[15] / max(s[1] + s[3], 1)
    print(f'Town01: {s[15]} of {s[1] + s[3]} accepted faces painted on their lane ({share:.3f}); small {s[2] + s[4]}; scan steps {s[0]}, '
          f'by small faces (0, 1-8, .., 41-48, 49-64) {s[5:13]}')
    assert rec is not None and rec['valid']                   # the second launch was a skipping one
    assert np.array_equal(first, ref) and np.array_equal(second, ref)
    assert share > 0.5


def test_another_resolution_does_not_take_the_path(ops, oracle):
    """192 x 192 with five keys runs four workgroups per CU, one item each: the plan switches the path off (tests/test_raster_plan_small_faces.py)
    and every face is queued"""
    from torchdrivesim_amd import _native as nat
    verts, faces, vcat = synthetic_map()
    cam_xy, psi = cameras()
    state, size, mask = scene(oracle, 1, 8, np.random.default_rng(7))
    ref = reference(ops, oracle, oracle_static(oracle, verts, faces, vcat, CATS), state, size, mask, cam_xy, psi, 192)
    with nat.testing() as T:
        smap = make_map(ops, verts, faces, vcat, CATS)
        try:
            T.tds_raster_set_debug(int(nat.RasterDebug.STATS))
            small_stats(T)
            img = render(ops, oracle, smap, state, size, mask, cam_xy, psi, 192).cpu().numpy()
            s = small_stats(T)
        finally:
            T.tds_raster_set_debug(0)
        del smap
    assert s[15] == 0 and s[2] > 0
    assert np.array_equal(img, ref)
