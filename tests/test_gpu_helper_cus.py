"""The helper enqueue of the persistent raster launch (include/tdship.h, tds_raster_aux_helper_t; csrc/tds_raster_plan.h, helper_grid): in
`Simulator.overlap_infractions = 'reserved'` mode the launch is enqueued a second time on the metric stream, so that the 32 CUs reserved for the metrics
render too once the metrics have ended.  Its workgroups take items from the same queues, so every image and coverage record here must be BYTE FOR BYTE
what the single launch leaves (`_ops.use_helper_cus = False`), and the metrics beside it what the serial order computes.  The bench's Town01 scene
at 256 x 256 with five keys, B = 8 x A = 64 = 512 cameras unless a case says otherwise; the module runs on the testing build with the threshold knob
at 0 (the product's 4 items per workgroup would give 512 cameras no helper), and its counters say which enqueue rendered how many items."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, A, FOV, RES = 8, 64, 35.0, 256


@pytest.fixture(scope='module')
def T():
    """the whole module runs on the testing build (the knob and the counters live there); everything the tests create dies before the switch back"""
    from torchdrivesim_amd import _native, _ops
    _ops.map_cache.clear()
    with _native.testing() as lib:
        assert lib.tds_raster_set_helper_min_items(0) == 0
        yield lib
        lib.tds_raster_set_debug(0)
        lib.tds_raster_set_helper_min_items(4)
        _ops.use_helper_cus = True
        _ops.map_cache.clear()


@pytest.fixture(scope='module')
def ops(T):
    from torchdrivesim_amd import _ops
    return _ops


@pytest.fixture(scope='module')
def streams(ops):
    rs, ms = ops.reserved_streams(torch.device(DEV))
    return rs, ms


def res_of(n):
    from torchdrivesim_amd.utils import Resolution
    return Resolution(n, n)


def item_counters(T):
    """(work items rendered by either enqueue, work items rendered by workgroups of the helper enqueue) since the last reading"""
    torch.cuda.synchronize()
    both, helper = (ctypes.c_ulonglong * 2)(), (ctypes.c_ulonglong * 1)()
    assert T.tds_raster_get_prep_stats(both) == 0 and T.tds_raster_get_helper_stats(helper) == 0
    return int(both[0]) + int(both[1]), int(helper[0])


def ring_loop(T, ops, streams, sim, actions, start, ring, helper, steps=4, metrics=True):
    """`steps` steps of the benchmark's loop on the raster stream, from state `start`, into the ring (whose coverage records are forgotten first: the first
    render into each buffer stores every line, the later ones skip) -> per step (image, coverage record or None, helper workgroups, items, helper items)"""
    from torchdrivesim_amd._native import RasterDebug as D
    rs, ms = streams
    ops.use_helper_cus = helper
    sim.overlap_infractions = 'reserved'
    sim.kinematic_model.set_state(start.clone())
    for buf in ring:
        ops.forget_coverage(buf)
    out = []
    T.tds_raster_set_debug(int(D.STATS))
    try:
        item_counters(T)
        with torch.cuda.stream(rs):
            for i in range(steps):
                sim.step(actions[i])
                buf = ring[i % len(ring)]
                img = sim.render_egocentric(res=res_of(RES), fov=FOV, out=buf)
                wgs = ops.last_helper_workgroups
                if metrics:
                    col, off = sim.compute_collision(), sim.compute_offroad()
                    if i >= 1 and sim.renderer.out_dtype == torch.float32:
                        assert col is sim._fork[3][('collision', None)][0]       # foreseen: on the metric stream ahead of the launch and of its helper
                rec = ops._owned_buffers[buf.data_ptr()]['record']
                items, helped = item_counters(T)
                out.append((img.clone(), None if rec is None else (rec['cov'].clone(), bool(rec['valid'])), wgs, items, helped))
    finally:
        T.tds_raster_set_debug(0)
        ops.use_helper_cus = True
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def world(T, ops):
    import bench
    sim, actions, _ = bench.build_simulator(B, A, torch.device(DEV), seed=9)
    return dict(sim=sim, actions=actions, start=sim.get_state().clone())


def compare(off, on, cus, n_items, tracked):
    for i, ((img0, rec0, wg0, items0, h0), (img1, rec1, wg1, items1, h1)) in enumerate(zip(off, on)):
        print(f'step {i}: helper workgroups {wg1}, items {items1} of which {h1} by helper workgroups (helper off: {items0}, {h0})')
        assert wg0 == 0 and h0 == 0 and items0 == n_items
        assert wg1 == 3 * cus                                              # three workgroups per CU of the metric stream
        assert items1 == n_items and 0 <= h1 <= n_items                    # items(main) + items(helper) == items: every item rendered once
        assert torch.equal(img0, img1), i
        assert bool(img1.flatten(2).amax(-1).gt(0).all())
        if tracked:
            assert rec0 is not None and rec1 is not None and rec0[1] and rec1[1]
            assert torch.equal(rec0[0], rec1[0]), i
        else:
            assert rec0 is None and rec1 is None


def metric_cus(ops, streams):
    return len(ops.stream_places(streams[1]))


def test_float32_ring_first_renders_and_skipping_renders(T, ops, streams, world):
    """four steps into a ring of two owned buffers, the metrics foreseen on the metric stream: renders 0 and 1 store every line, 2 and 3 skip the
    lines their record vouches for; images and records byte for byte those of the single launch"""
    ring = [ops.owned_image((B, A, 3, RES, RES), torch.float32, DEV) for _ in range(2)]
    off = ring_loop(T, ops, streams, world['sim'], world['actions'], world['start'], ring, helper=False)
    on = ring_loop(T, ops, streams, world['sim'], world['actions'], world['start'], ring, helper=True)
    cus = metric_cus(ops, streams)
    assert cus == 32
    compare(off, on, cus, B * A, tracked=True)
    del ring


def test_uint8_ring(T, ops, streams, world):
    """the same with uint8 output (no coverage record; a launch bound by instruction issue, for which 'reserved' foresees no metrics: the helper
    workgroups start with the launch)"""
    from torchdrivesim_amd.rendering import renderer_from_config
    from torchdrivesim_amd.rendering.hip import HipRendererConfig
    sim = world['sim']
    saved = sim.renderer
    sim.renderer = renderer_from_config(HipRendererConfig(out_dtype='uint8'), res=res_of(RES), fov=FOV)
    try:
        ring = [ops.owned_image((B, A, 3, RES, RES), torch.uint8, DEV) for _ in range(2)]
        off = ring_loop(T, ops, streams, sim, world['actions'], world['start'], ring, helper=False)
        on = ring_loop(T, ops, streams, sim, world['actions'], world['start'], ring, helper=True)
    finally:
        sim.renderer = saved
    compare(off, on, metric_cus(ops, streams), B * A, tracked=False)
    assert on[0][0].dtype == torch.uint8


def test_an_idle_helper_stream_renders_items_of_a_longer_launch(T, ops, streams):
    """2048 cameras (three items per workgroup of the main grid), nothing on the metric stream: the helper workgroups start with the launch and
    render some of its items -- so the equalities of this module are not those of a helper that never runs"""
    import bench
    sim, actions, _ = bench.build_simulator(32, A, torch.device(DEV), seed=10)
    start = sim.get_state().clone()
    ring = [ops.owned_image((32, A, 3, RES, RES), torch.float32, DEV)]
    off = ring_loop(T, ops, streams, sim, actions, start, ring, helper=False, steps=2, metrics=False)
    on = ring_loop(T, ops, streams, sim, actions, start, ring, helper=True, steps=2, metrics=False)
    compare(off, on, metric_cus(ops, streams), 32 * A, tracked=True)
    assert all(step[4] > 0 for step in on), [step[4] for step in on]


@pytest.mark.parametrize('own_stream', [False, True])
def test_metrics_beside_the_launch_and_its_helper_equal_the_serial_order(T, ops, streams, own_stream):
    """the loop of test_gpu_simulator.py::test_metrics_on_reserved_cus_beside_the_raster_launch with the helper on: the loop itself on the raster
    stream, or the library's detour from the caller's stream; images, collision and off-road equal the serial reference, step after step"""
    import bench
    sim, actions, _ = bench.build_simulator(B, A, torch.device(DEV), seed=9)
    ref, _, _ = bench.build_simulator(B, A, torch.device(DEV), seed=9)
    rs, ms = streams
    res = res_of(RES)
    sim.overlap_infractions = 'reserved'
    out = torch.empty(B, A, 3, RES, RES, device=DEV)
    cus = metric_cus(ops, streams)
    torch.cuda.synchronize()
    with (torch.cuda.stream(rs) if own_stream else contextlib.nullcontext()):
        for i in range(4):
            sim.step(actions[i])
            img = sim.render_egocentric(res=res, fov=FOV, out=out)
            assert ops.last_helper_workgroups == 3 * cus
            col, off = sim.compute_collision(), sim.compute_offroad()
            if i >= 1:
                assert col is sim._fork[3][('collision', None)][0]
            ref.step(actions[i])
            torch.cuda.current_stream().synchronize()
            ops.use_helper_cus = False
            try:
                want = ref.render_egocentric(res=res, fov=FOV)
            finally:
                ops.use_helper_cus = True
            assert ops.last_helper_workgroups == 0
            assert torch.equal(img, want)
            assert torch.equal(col, ref.compute_collision()) and torch.equal(off, ref.compute_offroad())
        img2 = sim.render_egocentric(res=res, fov=FOV)                      # without out=: the image comes from the pool
        assert torch.equal(img2, out)
    torch.cuda.synchronize()


# ---- calls that keep their single launch --------------------------------------------------------------------------------------------------
def single_launch(ops, streams, render):
    """render() on the raster stream with the switch on and off -> the image with it on; no helper either way, the same bytes"""
    with torch.cuda.stream(streams[0]):
        ops.use_helper_cus = True
        on = render()
        wgs = ops.last_helper_workgroups
        ops.use_helper_cus = False
        try:
            off = render()
        finally:
            ops.use_helper_cus = True
    torch.cuda.synchronize()
    assert wgs == 0
    assert torch.equal(on, off)
    return on


def test_a_differentiable_render_keeps_its_single_launch(T, ops, streams, world):
    sim = world['sim']
    sim.overlap_infractions = 'reserved'
    saved = world['start']

    def render():
        sim.kinematic_model.set_state(saved.clone().requires_grad_(True))
        img = sim.render_egocentric(res=res_of(RES), fov=FOV)
        assert img.requires_grad
        return img.detach()

    try:
        single_launch(ops, streams, render)
    finally:
        sim.kinematic_model.set_state(saved.clone())


def test_the_split_form_at_128_keeps_its_launches(T, ops, streams, world):
    sim = world['sim']
    sim.overlap_infractions = 'reserved'
    sim.kinematic_model.set_state(world['start'].clone())
    single_launch(ops, streams, lambda: sim.render_egocentric(res=res_of(128), fov=FOV).clone())


def test_32_cameras_at_the_product_threshold_keep_their_single_launch(T, ops, streams):
    """one item per workgroup of the main grid, the threshold at the product's 4: waiting for the metric stream could only delay the image"""
    import bench
    sim, actions, _ = bench.build_simulator(1, 32, torch.device(DEV), seed=9)
    sim.overlap_infractions = 'reserved'
    sim.step(actions[0])
    assert T.tds_raster_set_helper_min_items(4) == 0
    try:
        single_launch(ops, streams, lambda: sim.render_egocentric(res=res_of(RES), fov=FOV).clone())
    finally:
        T.tds_raster_set_helper_min_items(0)
    # ... and with the knob at 0 the same call takes the helper: the threshold was what kept it off
    with torch.cuda.stream(streams[0]):
        sim.render_egocentric(res=res_of(RES), fov=FOV)
        assert ops.last_helper_workgroups == 3 * metric_cus(ops, streams)
    torch.cuda.synchronize()


def test_a_helper_stream_that_is_the_calls_own_stream_is_not_used(T, ops, streams, world, monkeypatch):
    sim = world['sim']
    sim.overlap_infractions = 'reserved'
    sim.kinematic_model.set_state(world['start'].clone())
    plain = ops.raster_scene
    seen = []

    def own_stream_as_helper(*args, **kw):
        seen.append(kw.get('helper_stream'))
        kw['helper_stream'] = torch.cuda.current_stream(torch.device(DEV)) if kw.get('helper_stream') is not None else None
        return plain(*args, **kw)

    monkeypatch.setattr(ops, 'raster_scene', own_stream_as_helper)
    single_launch(ops, streams, lambda: sim.render_egocentric(res=res_of(RES), fov=FOV).clone())
    assert seen and seen[0] is not None and seen[0].cuda_stream == streams[1].cuda_stream        # the simulator did hand the metric stream down


def test_a_captured_render_keeps_its_single_launch_and_replays(T, ops, streams, world):
    """stream capture: the graph holds the one launch (no second branch to replay); the replay gives the eager image"""
    sim = world['sim']
    sim.overlap_infractions = 'reserved'
    sim.kinematic_model.set_state(world['start'].clone())
    res = res_of(RES)
    image = torch.empty(B, A, 3, RES, RES, device=DEV)
    ops.use_helper_cus = False
    try:
        want = sim.render_egocentric(res=res, fov=FOV).clone()
    finally:
        ops.use_helper_cus = True
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                     # eager warm-up on a side stream, as torch asks for before capture
        sim.render_egocentric(res=res, fov=FOV, out=image)
        assert ops.last_helper_workgroups > 0                      # (eager, through the detour: the helper is used)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sim.render_egocentric(res=res, fov=FOV, out=image)
        wgs = ops.last_helper_workgroups
    assert wgs == 0
    image.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(image, want)
