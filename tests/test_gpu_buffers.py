"""Where the rendered images live (csrc/alloc.hip, _ops.image_pool / owned_image): buffers whose physical pages are spread
out, handed to torch either through a memory pool (the reference-shaped `render_egocentric()` without `out=`) or as caller-owned tensors
(output rings).  No reference counterpart: rendering/cv2.py:52 allocates a numpy image per call."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_a_buffer_is_built_from_chunks_and_holds_data():
    from torchdrivesim_amd import _native as nat
    L = nat.lib()
    h = ctypes.c_void_p()
    nat.check(L.tds_buffer_create(1 << 30, 0, 0, ctypes.byref(h)), 'tds_buffer_create')
    n, chunks, spread = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    nat.check(L.tds_buffer_info(h, ctypes.byref(n), ctypes.byref(chunks), ctypes.byref(spread)), 'tds_buffer_info')
    assert (n.value, chunks.value, spread.value) == (1 << 30, 128, 1) and L.tds_buffer_ptr(h) % (2 << 20) == 0
    nat.check(L.tds_buffer_destroy(h), 'tds_buffer_destroy')
    nat.check(L.tds_buffer_create(1 << 20, 0, 0, ctypes.byref(h)), 'tds_buffer_create')            # small: one hipMalloc
    nat.check(L.tds_buffer_info(h, None, ctypes.byref(chunks), ctypes.byref(spread)), 'tds_buffer_info')
    assert (chunks.value, spread.value) == (0, 0)
    nat.check(L.tds_buffer_destroy(h), 'tds_buffer_destroy')
    assert L.tds_buffer_create(0, 0, 0, ctypes.byref(h)) == nat.E_INVAL and L.tds_buffer_create(1 << 20, 0, 64, ctypes.byref(h)) == nat.E_INVAL


def test_owned_image_is_a_tensor_over_library_memory():
    from torchdrivesim_amd import _ops
    free0, _ = torch.cuda.mem_get_info(DEV)
    before = torch.cuda.memory_allocated(DEV)
    t = _ops.owned_image((64, 8, 3, 256, 256), torch.float32, DEV)              # 402 MB
    assert t.shape == (64, 8, 3, 256, 256) and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    assert torch.cuda.memory_allocated(DEV) == before                            # not torch's allocator
    t.fill_(3.0)
    v = t[5, 2]                                                                  # a view keeps the buffer alive
    del t
    assert float(v.sum()) == 3.0 * 3 * 256 * 256
    del v
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(DEV)
    assert abs(free1 - free0) < (64 << 20)                                       # back with the driver


def test_images_without_out_come_from_the_pool_and_show_the_same_pixels():
    import bench
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.utils import Resolution
    sim, actions, _ = bench.build_simulator(32, 16, torch.device(DEV), seed=11)           # 32 x 16 x 3 x 256 x 256 x 4 = 403 MB >= SPREAD_MIN
    sim.step(actions[0])
    res = Resolution(256, 256)
    assert _ops.use_image_pool
    _ops.use_image_pool = False
    try:
        plain = sim.render_egocentric(res=res, fov=35.0)
    finally:
        _ops.use_image_pool = True
    img = sim.render_egocentric(res=res, fov=35.0)
    assert torch.equal(img, plain)
    ptr = img.data_ptr()
    assert ptr % (2 << 20) == 0                                                  # a block of its own, built by tds_torch_alloc
    del img
    again = sim.render_egocentric(res=res, fov=35.0)                              # the block is cached by torch's allocator like any other
    assert again.data_ptr() == ptr and torch.equal(again, plain)
    held = sim.render_egocentric(res=res, fov=35.0)                               # while `again` is alive: another block, never an alias
    assert held.data_ptr() != ptr and torch.equal(held, again)
    small = sim.render_egocentric(res=Resolution(64, 64), fov=35.0)               # below SPREAD_MIN: the default pool
    assert small.shape[-1] == 64
    del again, held
    _ops.release_image_pool()


def test_out_is_validated_with_real_errors():
    import bench
    from torchdrivesim_amd.utils import Resolution
    sim, actions, _ = bench.build_simulator(2, 4, torch.device(DEV), seed=1)
    res = Resolution(64, 64)
    good = torch.empty(2, 4, 3, 64, 64, device=DEV)
    assert sim.render_egocentric(res=res, out=good) is good
    for bad, word in ((torch.empty(2, 4, 3, 64, 32, device=DEV), 'shape'), (torch.empty(2, 4, 3, 64, 64, device=DEV, dtype=torch.uint8), 'float32'),
                      (torch.empty(2, 4, 3, 64, 128, device=DEV)[..., ::2], 'contiguous'),
                      (torch.empty(2 * 4 * 3 * 64 * 64 + 1, device=DEV)[1:].view(2, 4, 3, 64, 64), 'aligned')):
        with pytest.raises(RuntimeError, match=word):
            sim.render_egocentric(res=res, out=bad)


def test_the_workspace_is_sized_for_the_kernels_that_run():
    """tds_raster_scene_workspace_bytes_for: with the number of distinct keys known (tds_map_keys + the actors' keys) and at most
    15 of them the bit-plane kernels serve the launch -- face lists up to 144 x 144 (float32) / 208 x 208 (uint8), above nothing but the 64
    bytes of work queues -- instead of the 32 KB per camera that would serve every path."""
    import bench
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.utils import Resolution
    sim, actions, _ = bench.build_simulator(4, 16, torch.device(DEV), seed=2)
    keys = sim._scene()['map'].face_keys()
    assert keys is not None and 1 <= len(keys) <= 8 and len(set(keys)) == len(keys)
    _ops._workspaces.clear()
    img = sim.render_egocentric(res=Resolution(256, 256), fov=35.0)
    (ws,) = [w for w in _ops._workspaces.values() if w is not False]
    assert ws.numel() <= 4096, ws.numel()                                     # the persistent launch's queues, nothing else
    _ops._workspaces.clear()
    small = sim.render_egocentric(res=Resolution(64, 64), fov=35.0)
    (ws64,) = [w for w in _ops._workspaces.values() if w is not False]
    assert ws64.numel() >= 4 * 16 * 2048 * 16                                   # a list of 2 048 faces per camera for K3s + K3r
    assert bool(img.any()) and bool(small.any())
    # without the key count: the size that serves every path
    import ctypes
    from torchdrivesim_amd import _native as nat
    every, bits, u8hi = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    nat.call('tds_raster_scene_workspace_bytes', torch.device(DEV), 64, 256, ctypes.byref(every))
    nat.call('tds_raster_scene_workspace_bytes_for', torch.device(DEV), 64, 256, nat.OUT_F32, 5, ctypes.byref(bits))
    nat.call('tds_raster_scene_workspace_bytes_for', torch.device(DEV), 64, 256, nat.OUT_F32, 40, ctypes.byref(u8hi))
    assert bits.value <= 256 < every.value == u8hi.value


def test_a_headline_sized_buffer_is_built_in_seconds():
    """51.5 GB = the image of the headline shard: 6 144 chunks + their spacers, 12 k hipMemCreate and 6 k hipMemMap -- about a second on the
    boxes of rounds 4 and 5.  The time is printed so that the driver's log shows it (that run took 642 s and nothing said where)."""
    import time
    from torchdrivesim_amd import _native as nat
    L = nat.lib()
    h = ctypes.c_void_p()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nat.check(L.tds_buffer_create(1024 * 64 * 3 * 256 * 256 * 4, 0, 0, ctypes.byref(h)), 'tds_buffer_create')
    t1 = time.perf_counter()
    chunks, spread = ctypes.c_int64(), ctypes.c_int()
    nat.check(L.tds_buffer_info(h, None, ctypes.byref(chunks), ctypes.byref(spread)), 'tds_buffer_info')
    nat.check(L.tds_buffer_destroy(h), 'tds_buffer_destroy')
    t2 = time.perf_counter()
    print(f'tds_buffer_create(51.5 GB): {t1 - t0:.2f} s, destroy {t2 - t1:.2f} s, {chunks.value} chunks, spread {spread.value}')
    assert (chunks.value, spread.value) == (6144, 1)
    # (about 2.3 s here; the bound is generous on purpose -- a slow box must show up in the printed time, not as a red run that leaves every later test unrun)
    assert t1 - t0 < 30.0, f'building a 51.5 GB buffer took {t1 - t0:.1f} s'


def test_a_buffer_that_does_not_fit_with_its_spacers_is_built_dense_and_nothing_leaks():
    """create_spread's low-memory branch (alloc.hip: the spacers are given back when hipMemCreate runs out) and tds_torch_alloc's dense fallback:
    with most of the device held, a buffer that fits only WITHOUT spacers must still come (its tail as dense as a hipMalloc), one that does not
    fit at all must fail with TDS_ENOMEM, and either way the driver has all of it back afterwards."""
    from torchdrivesim_amd import _native as nat
    L = nat.lib()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    free0, total = torch.cuda.mem_get_info(DEV)
    if free0 < 0.9 * total:
        # the test takes all free device memory but 9 GB: only with the device to itself (another process allocating meanwhile would make it
        # fail for reasons that are not the library's -- ADVICE r5)
        pytest.skip(f'the device is shared: {free0 / 2 ** 30:.0f} of {total / 2 ** 30:.0f} GiB free')
    want = 6 << 30
    # leave room for the buffer and half of its spacers: the spacer chunks run out on the way
    hold_bytes = free0 - want - (want // 2)
    assert hold_bytes > 0
    hold = ctypes.c_void_p()
    nat.check(L.tds_buffer_create(hold_bytes, 0, nat.BUFFER_DENSE, ctypes.byref(hold)), 'tds_buffer_create(dense)')
    try:
        free1, _ = torch.cuda.mem_get_info(DEV)
        assert free1 < want * 2
        h = ctypes.c_void_p()
        nat.check(L.tds_buffer_create(want, 0, 0, ctypes.byref(h)), 'tds_buffer_create')
        n, chunks, spread = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        nat.check(L.tds_buffer_info(h, ctypes.byref(n), ctypes.byref(chunks), ctypes.byref(spread)), 'tds_buffer_info')
        assert n.value == want and chunks.value == want >> 23 and spread.value == 1
        # the memory is usable end to end
        probe = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        ptr = L.tds_buffer_ptr(h)
        L_hip = ctypes.CDLL('libamdhip64.so')
        for off in (0, want // 2, want - (1 << 20)):
            assert L_hip.hipMemset(ctypes.c_void_p(ptr + off), 0x5a, ctypes.c_size_t(1 << 20)) == 0
            assert L_hip.hipMemcpy(ctypes.c_void_p(probe.data_ptr()), ctypes.c_void_p(ptr + off), ctypes.c_size_t(1 << 20), 3) == 0
            assert int(probe.min()) == 0x5a == int(probe.max())
        # nothing at all is left for a second one: TDS_ENOMEM, and what the attempt took on the way is given back
        free2, _ = torch.cuda.mem_get_info(DEV)
        h2 = ctypes.c_void_p()
        rc = L.tds_buffer_create(free2 + (4 << 30), 0, 0, ctypes.byref(h2))
        assert rc == nat.E_NOMEM and not h2.value, rc
        free3, _ = torch.cuda.mem_get_info(DEV)
        assert free3 > free2 - (64 << 20)
        # the entry point torch's pluggable allocator binds: same size, spread impossible -> falls back, or reports out of memory with a null
        p = L.tds_torch_alloc(ctypes.c_size_t(free2 + (4 << 30)), 0, None)
        assert not p
        free4, _ = torch.cuda.mem_get_info(DEV)
        assert free4 > free2 - (64 << 20)
        nat.check(L.tds_buffer_destroy(h), 'tds_buffer_destroy')
    finally:
        nat.check(L.tds_buffer_destroy(hold), 'tds_buffer_destroy')
    torch.cuda.synchronize()
    free5, _ = torch.cuda.mem_get_info(DEV)
    assert free5 > free0 - (128 << 20)                                           # nothing is left behind (other users of the device may have freed more)
