"""The persistent bit-plane launch computes each work item's scan set-up (trim polygon, grid window, grid rows) once, in camera_prepare_kernel in
front of it, and its workgroups load the record (raster.hip; include/tdship.h, tds_raster_aux_t::camera_prep).  The record is computed by the very
functions the raster kernel uses, so every image here must be BYTE FOR BYTE the one rendered without the table (`_ops.use_camera_prep = False`), and
equal to the oracle where the parity tests hold that shape to it.  Every case also reads the two counters of the testing build (work items that used
their record / that computed the set-up in the kernel), so no case passes because the table was silently ignored.  The bench's Town01 scene at
B = 2 x A = 8 (16 cameras) unless a case says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, A, FOV = 2, 8, 35.0
RECORD_WORDS = 84          # 336 bytes: camera + polygon (12 floats), window (4), entries, flags, 2 unused, 16 rows of 4


@pytest.fixture(scope='module')
def T():
    """the whole module runs on the testing build (the counters live there); everything the tests create dies before the switch back"""
    from torchdrivesim_amd import _native
    with _native.testing() as lib:
        yield lib
        lib.tds_raster_set_debug(0)
        lib.tds_raster_set_strip_width(0)


@pytest.fixture(scope='module')
def ops(T):
    from torchdrivesim_amd import _ops
    _ops._camera_preps.clear()         # (tables sized under another module's knobs of the testing build: too small a table is never an error, but
    yield _ops                         #  its items would compute in the kernel, and the counters here would say so)
    _ops.use_camera_prep = True
    _ops._camera_preps.clear()


@pytest.fixture(scope='module')
def world(T, ops):
    import bench
    sim, actions, host = bench.build_simulator(B, A, torch.device(DEV), seed=11)
    sim.step(actions[0])
    return dict(sim=sim, actions=actions, host=host)


def res_of(n):
    from torchdrivesim_amd.utils import Resolution
    return Resolution(n, n)


def counters(T):
    """(items that used their record, items that computed in the kernel) since the last reading"""
    torch.cuda.synchronize()
    out = (ctypes.c_ulonglong * 2)()
    assert T.tds_raster_get_prep_stats(out) == 0
    return int(out[0]), int(out[1])


def on_and_off(T, ops, render, debug=0):
    """render() with the table on and off -> (image, counters with the table on, counters with it off); the images are equal, byte for byte, and
    without the table no item uses a record"""
    from torchdrivesim_amd._native import RasterDebug as D
    T.tds_raster_set_debug(int(D.STATS) | int(debug))
    try:
        counters(T)
        ops.use_camera_prep = True
        on = render()
        c_on = counters(T)
        ops.use_camera_prep = False
        off = render()
        c_off = counters(T)
    finally:
        ops.use_camera_prep = True
        T.tds_raster_set_debug(0)
    assert c_off[0] == 0, c_off
    assert on.data_ptr() != off.data_ptr() and torch.equal(on, off)
    assert bool(on.flatten(2).amax(-1).gt(0).any())
    return on, c_on, c_off


def oracle_image(oracle, world, res, fov):
    """the oracle's image of the module's scene (computed once: the tests that move the agents put them back)"""
    if ('oracle', res, fov) not in world:
        world['oracle', res, fov] = _oracle_image(oracle, world, res, fov)
    return world['oracle', res, fov]


def _oracle_image(oracle, world, res, fov):
    sim = world['sim']
    state0, size, present, act, verts, faces, vcat, cats = world['host']
    s = sim.get_state()
    sn = s.cpu().numpy()
    sc = torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1).cpu().numpy()
    sv, sa, sf = oracle.static_mesh_arrays(verts, faces, vcat, cats)
    mask = np.ascontiguousarray(np.broadcast_to(present[:, None, :], (B, A, A)))
    return oracle.render_scenes(sn, size, mask, sn[..., :2].copy(), sc, sv, sa, sf, fov, res, agent_sc=sc)


@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_the_headline_shape_uses_every_record_and_equals_the_oracle(T, ops, world, oracle, dtype):
    """256 x 256, five keys: the instantiation of the headline (and its uint8 twin) -- all 16 items use their record"""
    sim = world['sim']
    sim.renderer.cfg.out_dtype = dtype
    try:
        img, c_on, c_off = on_and_off(T, ops, lambda: sim.render_egocentric(res=res_of(256), fov=FOV))
    finally:
        sim.renderer.cfg.out_dtype = 'float32'
    assert c_on == (B * A, 0) and c_off == (0, B * A), (c_on, c_off)
    assert img.dtype == getattr(torch, dtype)
    assert np.array_equal(img.cpu().numpy(), oracle_image(oracle, world, 256, FOV).astype(img.cpu().numpy().dtype))


def test_two_strips_have_a_record_each(T, ops, world, oracle):
    """256 x 256 cut into two strips of 128 columns (the strip-width knob) for the persistent instantiation: 32 items, all use their record; the records of a camera's two strips
    share the camera and differ in the scan window"""
    from torchdrivesim_amd._native import RasterDebug as D
    sim = world['sim']
    T.tds_raster_set_strip_width(128)
    ops._camera_preps.clear()          # (the table's size is cached per shape; the knob of the testing build changes it behind the cache)
    try:
        # (MINWG3: strips this narrow would go to the instantiation for four workgroups per CU, which takes no table)
        img, c_on, c_off = on_and_off(T, ops, lambda: sim.render_egocentric(res=res_of(256), fov=FOV), debug=D.MINWG3)
        tabs = [t for t in ops._camera_preps.values() if t is not False and t.numel() == 2 * B * A * RECORD_WORDS * 4]
    finally:
        T.tds_raster_set_strip_width(0)
        ops._camera_preps.clear()
    assert c_on == (2 * B * A, 0) and c_off == (0, 2 * B * A), (c_on, c_off)
    assert len(tabs) == 1
    rec = tabs[0].view(torch.int32).view(B * A, 2, RECORD_WORDS).cpu()
    assert torch.equal(rec[:, 0, :12], rec[:, 1, :12])                           # one camera, one trim polygon
    assert bool((rec[:, 0, 12:17] != rec[:, 1, 12:17]).any(-1).all())            # two windows: cell rectangle or entries differ
    assert int(rec[:, :, 17].abs().max()) == 0                                    # none flagged
    assert np.array_equal(img.cpu().numpy(), oracle_image(oracle, world, 256, FOV))


def test_a_camera_off_the_map_and_one_over_its_edge(T, ops, world):
    """no grid row at all (the record says so: nothing of the map is scanned) and a window that the map's edge clips"""
    sim = world['sim']
    verts = world['host'][4]
    saved = sim.get_state().clone()
    s = saved.clone()
    s[0, 0, :2] = 1.0e6
    s[0, 1, 0], s[0, 1, 1] = float(verts[:, 0].min()), float(verts[:, 1].min())
    s[1, 0, 0], s[1, 0, 1] = float(verts[:, 0].max()) + 10.0, float(verts[:, 1].max()) - 5.0
    sim.kinematic_model.set_state(s)
    try:
        img, c_on, c_off = on_and_off(T, ops, lambda: sim.render_egocentric(res=res_of(256), fov=FOV))
    finally:
        sim.kinematic_model.set_state(saved)
    assert c_on == (B * A, 0), c_on
    assert float(img[0, 0].amax()) > 0          # the far camera still sees itself
    assert float(img[0, 1].amax()) > 0 and float(img[1, 0].amax()) > 0


@pytest.fixture(scope='module')
def fine_grid(T, ops):
    """the same scene over a StaticMap with 4 m grid cells, every agent within a few metres of the middle of the map"""
    import bench
    orig = ops.StaticMap.__init__
    ops.StaticMap.__init__ = lambda self, *a, **k: orig(self, *a, **{**k, 'cell_size': 4.0})
    ops.map_cache.clear()                                            # (maps are cached by content: not the one the other tests built)
    try:
        sim, actions, host = bench.build_simulator(B, A, torch.device(DEV), seed=12)
        verts = host[4]
        mid = torch.tensor([float(verts[:, 0].min() + verts[:, 0].max()) / 2, float(verts[:, 1].min() + verts[:, 1].max()) / 2], device=DEV)
        s = sim.get_state().clone()
        gen = torch.Generator(device='cpu').manual_seed(5)
        s[..., :2] = mid + (torch.rand(B, A, 2, generator=gen).to(DEV) * 16.0 - 8.0)
        s[..., 2] = (torch.rand(B, A, generator=gen).to(DEV) * 2 - 1) * float(np.pi)
        s[0, 0, 2], s[0, 1, 2] = 0.0, float(np.pi / 4)
        sim.kinematic_model.set_state(s)
        sim.render_egocentric(res=res_of(256), fov=FOV)              # builds the map while the cell size is forced
        torch.cuda.synchronize()
    finally:
        ops.StaticMap.__init__ = orig
        ops.map_cache.clear()                                        # ... and no later simulator gets this one
    return sim


def test_more_grid_rows_than_a_record_holds_are_computed_in_the_kernel(T, ops, fine_grid):
    """4 m cells under a 100 m view: at least 25 grid rows per camera, a record holds 16 -- every item is flagged and computes, as before"""
    img, c_on, c_off = on_and_off(T, ops, lambda: fine_grid.render_egocentric(res=res_of(256), fov=100.0))
    assert c_on == (0, B * A) and c_off == (0, B * A), (c_on, c_off)


def test_the_same_fine_grid_under_a_35_m_view_uses_the_records(T, ops, fine_grid):
    """... and 9 to 14 rows under a 35 m view (35 m x sqrt 2 at 45 degrees, 2 px margin): records again"""
    img, c_on, c_off = on_and_off(T, ops, lambda: fine_grid.render_egocentric(res=res_of(256), fov=FOV))
    assert c_on == (B * A, 0), c_on


def test_a_two_town_map_set(T, ops):
    """every scene's record comes from its own town's grid (a.views / scene_map in camera_prepare_kernel as in scan_init)"""
    import bench
    sim, actions, _ = bench.build_simulator(4, A, torch.device(DEV), seed=13, mixed=True)
    sim.step(actions[0])
    img, c_on, c_off = on_and_off(T, ops, lambda: sim.render_egocentric(res=res_of(256), fov=FOV))
    assert c_on[0] + c_on[1] == 4 * A and c_on[0] > 0, c_on
    assert bool(img.flatten(2).amax(-1).gt(0).all())


def test_a_differentiable_call(T, ops, world):
    """the instantiation that also stores the index slices is a persistent launch too and takes the table when it is given one
    (`_ops.use_camera_prep_with_slices`); by default the Python layer gives it none: that launch stores every line, and the table made it slower"""
    sim = world['sim']
    saved = sim.get_state().clone()

    def render():
        s = saved.clone().requires_grad_(True)
        sim.kinematic_model.set_state(s)
        img = sim.render_egocentric(res=res_of(256), fov=FOV)
        assert img.requires_grad
        return img.detach()

    try:
        img0, c_default, _ = on_and_off(T, ops, render)
        ops.use_camera_prep_with_slices = True
        img, c_on, c_off = on_and_off(T, ops, render)
    finally:
        ops.use_camera_prep_with_slices = False
        sim.kinematic_model.set_state(saved)
    assert c_default == (0, B * A), c_default
    assert c_on == (B * A, 0) and c_off == (0, B * A), (c_on, c_off)
    assert torch.equal(img, img0)


def test_a_ring_of_two_owned_buffers_with_write_skipping(T, ops, world):
    """four steps into a ring of two buffers, once with the table and once without: the same images, and the coverage record is kept either way.
    This is the one case whose aux carries the coverage record AND the table (the first two renders store every line -- TDS_RASTER_REWRITE_ALL --,
    the next two skip): with the table on all B * A items of every render use their record and none computes in the kernel, with it off the
    reverse -- the table is not dropped because a coverage record is there"""
    from torchdrivesim_amd._native import RasterDebug as D
    sim, actions = world['sim'], world['actions']
    saved = sim.get_state().clone()
    shape = (B, A, 3, 256, 256)
    rings = {True: [ops.owned_image(shape, device=DEV) for _ in range(2)], False: [ops.owned_image(shape, device=DEV) for _ in range(2)]}
    T.tds_raster_set_debug(int(D.STATS))
    try:
        for i in range(4):
            sim.step(actions[1 + i])
            want = sim.render_egocentric(res=res_of(256), fov=FOV)
            counters(T)                                    # (the items of the render above are not the ring's)
            for table in (True, False):
                ops.use_camera_prep = table
                buf = rings[table][i % 2]
                got = sim.render_egocentric(res=res_of(256), fov=FOV, out=buf)
                assert counters(T) == ((B * A, 0) if table else (0, B * A)), (i, table)
                rec = ops._owned_buffers[buf.data_ptr()]['record']
                assert rec is not None and rec['valid'], (i, table)               # coverage_maintained, as without the table
                assert torch.equal(got, want), (i, table)
            assert torch.equal(rings[True][i % 2], rings[False][i % 2])
    finally:
        ops.use_camera_prep = True
        T.tds_raster_set_debug(0)
        sim.kinematic_model.set_state(saved)
        del rings


def test_shapes_that_other_instantiations_serve_take_no_table(T, ops, world):
    """192 x 192 with five keys (four workgroups per CU) and six keys at 256 x 256 (8-wave workgroups) keep their code: the host passes them no
    table, and no item reports a record"""
    sim = world['sim']
    img, c_on, c_off = on_and_off(T, ops, lambda: sim.render_egocentric(res=res_of(192), fov=FOV))
    assert c_on[0] == 0, c_on
    import bench
    six, actions, _ = bench.build_simulator(B, A, torch.device(DEV), seed=14)
    six._agent_types = ['vehicle', 'pedestrian']
    six.agent_type = six.agent_type.clone()
    six.agent_type[:, ::2] = 1
    six._scene_cache = None
    img, c_on, c_off = on_and_off(T, ops, lambda: six.render_egocentric(res=res_of(256), fov=FOV))
    assert c_on[0] == 0, c_on


def test_a_captured_step_and_render_follow_the_poses(T, ops):
    """the prepare kernel is an ordinary launch of the captured stream: a replay after the poses changed prepares the new cameras"""
    import bench
    from torchdrivesim_amd._native import RasterDebug as D
    dev = torch.device(DEV)
    sim, actions, _ = bench.build_simulator(B, A, dev, seed=15)
    ref, _, _ = bench.build_simulator(B, A, dev, seed=15)
    state = sim.get_state().clone()
    action = actions[0].clone()
    image = torch.empty(B, A, 3, 256, 256, device=dev)

    def step():
        sim.kinematic_model.set_state(state)
        sim.step(action)
        return sim.render_egocentric(res=res_of(256), fov=FOV, out=image), sim.get_state()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    T.tds_raster_set_debug(int(D.STATS))
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            img, new = step()
            state_next = new.clone()
        counters(T)
        seen = []
        for i in range(3):
            action.copy_(actions[i])
            g.replay()
            assert counters(T) == (B * A, 0)
            ops.use_camera_prep = False
            ref.kinematic_model.set_state(state.clone())
            ref.step(actions[i])
            want = ref.render_egocentric(res=res_of(256), fov=FOV)
            ops.use_camera_prep = True
            counters(T)                                   # (the reference's items computed in the kernel: not the replay's)
            assert torch.equal(img, want), i
            seen.append(img.clone())
            state.copy_(state_next)
        assert not torch.equal(seen[0], seen[2])
    finally:
        ops.use_camera_prep = True
        T.tds_raster_set_debug(0)


def test_a_struct_that_does_not_say_it_has_the_fields_gets_no_table(T, ops, world, monkeypatch):
    """the two fields are appended to tds_raster_aux_t and read only under TDS_RASTER_HAS_CAMERA_PREP: the same call without the flag (what a
    caller built against the shorter struct sends) computes every set-up in the kernel, and paints the same image"""
    from torchdrivesim_amd import _native as nat
    from torchdrivesim_amd._native import RasterDebug as D
    sim = world['sim']
    want = sim.render_egocentric(res=res_of(256), fov=FOV)
    T.tds_raster_set_debug(int(D.STATS))
    try:
        counters(T)
        monkeypatch.setattr(nat, 'RASTER_HAS_CAMERA_PREP', 0)
        got = sim.render_egocentric(res=res_of(256), fov=FOV)
        assert counters(T) == (0, B * A)
    finally:
        T.tds_raster_set_debug(0)
    assert torch.equal(got, want)
