"""The persistent 4-wave bit-plane launches leave a work item's agents to ONE wave of the workgroup (raster.hip: scan_step, ACTW;
tds_actor_lanes.h): one lane per agent for the distance cull, three lanes per VISIBLE agent for the faces, the masked agents' dot once.  Every case
here renders the same launch twice on the testing build -- as the product does, and with TDS_RASTER_DBG_NO_ACTOR_WAVE, which gives the per-wave
phases back -- and the two results must be equal byte for byte, in every image; where the oracle serves the scene the image equals the oracle's too.
The testing build's counter says how many work items had their agents served by the actor wave: all of them, and none with the flag, so no case
passes because the path was silently not taken.  256 x 256 throughout: the smallest side at which the persistent instantiation is what runs.
Town01; B = 2 scenes, the cameras at four of the agents (the first, two in between, the last: with 130 agents they sit in all three rounds of 64)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_parity import LEVELS, actor_keys, dev, make_map, oracle_static, pack, sc_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, FOV, RES = 2, 35.0, 256
COUNTS = (1, 2, 21, 22, 64, 65, 130)


@pytest.fixture(scope='module')
def T():
    """the whole module runs on the testing build (the flag and the counter live there); everything the tests create dies before the switch back"""
    from torchdrivesim_amd import _native, _ops
    _ops.map_cache.clear()
    _ops._camera_preps.clear()
    with _native.testing() as lib:
        yield lib
        lib.tds_raster_set_debug(0)
        lib.tds_raster_set_strip_width(0)
        lib.tds_raster_set_helper_min_items(4)
        _ops.map_cache.clear()
        _ops._camera_preps.clear()


@pytest.fixture(scope='module')
def ops(T):
    from torchdrivesim_amd import _ops
    return _ops


@pytest.fixture(scope='module')
def town(T, ops, oracle):
    import bench
    t = load_golden('town01_mesh.npz')
    verts, faces, vcat, cats = t['verts'], t['faces'], t['vert_category'], [str(c) for c in t['categories']]
    smap = make_map(ops, verts, faces, vcat, cats)
    centres = bench.synth_agents(B, 1, verts[vcat == cats.index('road')], 77)[0][:, 0, :2]      # a point on a road per scene
    return dict(smap=smap, static=oracle_static(oracle, verts, faces, vcat, cats), centres=centres, refs={})


def served(T):
    torch.cuda.synchronize()
    out = (ctypes.c_ulonglong * 1)()
    assert T.tds_raster_get_actor_wave_stats(out) == 0
    return int(out[0])


def both(T, call, items, debug=0):
    """call() as the product runs it and with the per-wave phases -> the former's result(s), after holding the two equal in every image"""
    from torchdrivesim_amd._native import RasterDebug as D
    try:
        T.tds_raster_set_debug(int(D.STATS) | int(debug))
        served(T)
        on = call()
        n_on = served(T)
        T.tds_raster_set_debug(int(D.STATS) | int(D.NO_ACTOR_WAVE) | int(debug))
        off = call()
        n_off = served(T)
    finally:
        T.tds_raster_set_debug(0)
    assert items is None or (n_on, n_off) == (items, 0), (n_on, n_off, items)
    tup = lambda r: tuple(t for t in (r if isinstance(r, tuple) else (r,)) if isinstance(t, torch.Tensor))
    for x, y in zip(tup(on), tup(off)):
        assert x.data_ptr() != y.data_ptr()
        if x.dim() < 3:                                       # (the index slices: one flat buffer)
            assert torch.equal(x, y)
            continue
        differ = (x != y).flatten(2).any(-1)
        assert not bool(differ.any()), f'{int(differ.sum())} of {differ.numel()} images differ'
    return on


def scene(town, A, kind, seed=1):
    """crowd: every agent within 8 m of the scene's centre -- each camera sees them all; spread: 1 km apart -- each camera sees itself alone"""
    gen = np.random.default_rng(1000 * A + seed)
    xy = np.zeros((B, A, 2))
    if kind == 'crowd':
        r, th = 8.0 * np.sqrt(gen.uniform(0, 1, (B, A))), gen.uniform(0, 2 * np.pi, (B, A))
        xy = town['centres'][:, None] + np.stack([r * np.cos(th), r * np.sin(th)], -1)
    else:
        xy[..., 0] = town['centres'][:, None, 0] + 1000.0 * np.arange(A)[None]
        xy[..., 1] = town['centres'][:, None, 1]
    state = np.concatenate([xy, gen.uniform(-np.pi, np.pi, (B, A, 1)), np.zeros((B, A, 1))], -1).astype(np.float32)
    size = (np.array([4.5, 2.0]) * gen.uniform(0.9, 1.1, (B, A, 2))).astype(np.float32)
    cams = sorted({0, A // 3, (2 * A) // 3, A - 1})
    return dict(state=state, size=size, cams=cams, cam_xy=state[:, cams, :2].copy(), psi=state[:, cams, 2].copy(), mask=np.ones((B, len(cams), A), bool))


def render(ops, oracle, town, sc, dtype=torch.float32, keys=None, **kw):
    sd = dev(sc['state'])
    keys = actor_keys(town['smap'], *sc['state'].shape[:2]) if keys is None else keys
    return ops.raster_scene(town['smap'], sd, ops.heading_sc(sd[..., 2]), dev(oracle.actor_template(sc['size'])), keys, dev(sc['mask']), dev(sc['cam_xy']),
                            ops.heading_sc(dev(sc['psi'])), FOV, RES, dtype, **kw)


def reference(ops, oracle, town, sc, key):
    """the oracle's images of a scene, computed once per scene"""
    if key not in town['refs']:
        sv, sa, sf = town['static']
        town['refs'][key] = oracle.render_scenes(sc['state'], sc['size'], sc['mask'], sc['cam_xy'], sc_np(ops.heading_sc(dev(sc['psi']))), sv, sa, sf, FOV, RES,
                                                 agent_sc=sc_np(ops.heading_sc(dev(sc['state'][..., 2]))))
    return town['refs'][key]


def n_img(sc):
    return B * len(sc['cams'])


@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
@pytest.mark.parametrize('kind', ['crowd', 'spread'])
@pytest.mark.parametrize('A', COUNTS)
def test_crowds_and_spreads_equal_the_per_wave_phases_and_the_oracle(T, ops, oracle, town, A, kind, dtype):
    """a crowd of 22 / 64 and more takes two / three and more face steps per round, 65 and 130 agents a second and a third round; in a spread the
    actor wave projects the camera's own agent alone"""
    sc = scene(town, A, kind)
    img = both(T, lambda: render(ops, oracle, town, sc, getattr(torch, dtype)), n_img(sc)).cpu().numpy()
    ref = reference(ops, oracle, town, sc, (A, kind))
    assert np.array_equal(img, ref.astype(img.dtype)), int((img != ref).any((2, 3, 4)).sum())
    assert bool((img.reshape(n_img(sc), -1).max(-1) > 0).all())


@pytest.mark.parametrize('masked', ['others', 'all'])
@pytest.mark.parametrize('A', [22, 65])
def test_masked_agents_and_their_dot(T, ops, oracle, town, A, masked):
    """every agent but the camera's own masked, and every agent masked: the dot alone is painted, and once (the per-wave phases paint the same dot
    from up to four waves; the planes are OR-ed)"""
    sc = scene(town, A, 'crowd')
    sc['mask'][:] = False
    if masked == 'others':
        for k, a in enumerate(sc['cams']):
            sc['mask'][:, k, a] = True
    img = both(T, lambda: render(ops, oracle, town, sc), n_img(sc)).cpu().numpy()
    ref = reference(ops, oracle, town, sc, (A, 'crowd', masked))
    assert np.array_equal(img, ref), int((img != ref).any((2, 3, 4)).sum())
    unmasked = reference(ops, oracle, town, scene(town, A, 'crowd'), (A, 'crowd'))
    assert not np.array_equal(ref, unmasked)


def test_a_nan_pose_is_kept(T, ops, oracle, town):
    sc = scene(town, 22, 'crowd')
    sc['state'][0, 1, 0] = np.nan
    sc['state'][1, 5, 1] = np.nan
    both(T, lambda: render(ops, oracle, town, sc), n_img(sc))


def test_a_part_without_a_key_and_keys_per_camera(T, ops, oracle, town):
    """key 0: the agent has no direction triangle (or no body); (B, Nc, N, 2) keys: every camera sees its own colours"""
    sc = scene(town, 65, 'crowd')
    keys = actor_keys(town['smap'], B, 65).clone()
    keys[:, ::3, 1] = 0
    keys[:, 5::7, 0] = 0
    plain = render(ops, oracle, town, sc)
    img = both(T, lambda: render(ops, oracle, town, sc, keys=keys), n_img(sc))
    assert not torch.equal(img, plain)
    # (no new key: a sixth would hand the launch to the 8-wave instantiation) camera 1 sees bodies and direction triangles in each other's key
    per_cam = keys[:, None].repeat(1, len(sc['cams']), 1, 1).contiguous()
    per_cam[:, 1] = per_cam[:, 1].flip(-1)
    img2 = both(T, lambda: render(ops, oracle, town, sc, keys=per_cam), n_img(sc))
    assert torch.equal(img2[:, 0], img[:, 0]) and not torch.equal(img2[:, 1], img[:, 1])


def extras(town, sc, K, seed=3):
    gen = np.random.default_rng(seed)
    Nc = len(sc['cams'])
    base = sc['cam_xy'][:, :, None, None, :] + gen.uniform(-15, 15, (B, Nc, K, 1, 2))
    tri = (base + gen.uniform(-0.8, 0.8, (B, Nc, K, 3, 2))).astype(np.float32)
    key = np.full((B, Nc, K), int(actor_keys(town['smap'], 1, 1)[0, 0, 1]), np.int64)      # (the direction triangles' key: a sixth key would hand the
                                                                                             # launch to the 8-wave instantiation)
    key[:, :, ::5] = 0
    return dev(tri), dev(key).to(torch.int32)


@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_per_camera_triangles_stay_on_every_wave(T, ops, oracle, town, dtype):
    """waypoint discs (SceneArgsEx): the other three waves start with them, the actor wave reaches them after the dot"""
    sc = scene(town, 22, 'crowd')
    sc['mask'][:, :, 3] = False
    tri, key = extras(town, sc, 300)
    plain = render(ops, oracle, town, sc, getattr(torch, dtype))
    img = both(T, lambda: render(ops, oracle, town, sc, getattr(torch, dtype), extra_tri=tri, extra_key=key), n_img(sc))
    assert not torch.equal(img, plain)


def test_two_strips_of_128_columns(T, ops, oracle, town):
    """the strip-width knob with MINWG3 (strips this narrow would go to the instantiation for four workgroups per CU): two work items per
    camera, each with an actor wave of its own"""
    from torchdrivesim_amd._native import RasterDebug as D
    sc = scene(town, 65, 'crowd')
    T.tds_raster_set_strip_width(128)
    ops._camera_preps.clear()
    try:
        img = both(T, lambda: render(ops, oracle, town, sc), 2 * n_img(sc), debug=D.MINWG3).cpu().numpy()
    finally:
        T.tds_raster_set_strip_width(0)
        ops._camera_preps.clear()
    assert np.array_equal(img, reference(ops, oracle, town, sc, (65, 'crowd')))


def test_nine_keys_in_two_strips(T, ops, oracle, town):
    """four more body colours: nine keys, which the plan cuts into two strips of 128 columns at three workgroups per CU"""
    sc = scene(town, 22, 'crowd')
    keys = actor_keys(town['smap'], B, 22).clone()
    rank = town['smap'].rank_of(LEVELS['vehicle']) << 24
    for k, rgb in enumerate([(200, 10, 10), (10, 200, 10), (10, 10, 200), (200, 200, 10)]):
        keys[:, 1 + k::5, 0] = rank | pack(rgb)
    img = both(T, lambda: render(ops, oracle, town, sc, keys=keys), 2 * n_img(sc))
    assert len(torch.unique(img.flatten(3).permute(0, 1, 3, 2).reshape(-1, 3), dim=0)) >= 8


def test_a_camera_off_the_map(T, ops, oracle, town):
    sc = scene(town, 22, 'spread')
    sc['state'][0, 0, :2] = 1.0e6
    sc['cam_xy'][0, 0] = 1.0e6
    img = both(T, lambda: render(ops, oracle, town, sc), n_img(sc))
    assert float(img[0, 0].amax()) > 0          # the far camera still sees itself


def test_a_two_town_map_set(T, ops):
    import bench
    from torchdrivesim_amd.utils import Resolution
    sim, actions, _ = bench.build_simulator(4, 8, torch.device(DEV), seed=13, mixed=True)
    sim.step(actions[0])
    img = both(T, lambda: sim.render_egocentric(res=Resolution(RES, RES), fov=FOV), 4 * 8)
    assert bool(img.flatten(2).amax(-1).gt(0).all())


def test_the_helper_enqueue_on_a_second_stream(T, ops, oracle, town):
    """the workgroups of the second enqueue take items like the others: each item has one actor wave, whichever enqueue rendered it"""
    sc = scene(town, 65, 'crowd')
    rs, ms = ops.reserved_streams(torch.device(DEV))
    assert T.tds_raster_set_helper_min_items(0) == 0
    seen = []

    def call():
        torch.cuda.synchronize()
        with torch.cuda.stream(rs):
            img = render(ops, oracle, town, sc, helper_stream=ms)
            seen.append(ops.last_helper_workgroups)
        torch.cuda.synchronize()
        return img

    try:
        img = both(T, call, n_img(sc)).cpu().numpy()
    finally:
        T.tds_raster_set_helper_min_items(4)
    assert seen[0] > 0 and seen[1] > 0, seen
    assert np.array_equal(img, reference(ops, oracle, town, sc, (65, 'crowd')))


def test_a_differentiable_call(T, ops, oracle, town):
    """the instantiation that also stores the index slices: the image and the slices"""
    sc = scene(town, 65, 'crowd')
    sc['mask'][:, :, 7] = False
    img, slices, keys = both(T, lambda: render(ops, oracle, town, sc, index_slices=True), n_img(sc))
    assert slices is not None and keys is not None
    assert torch.equal(img, render(ops, oracle, town, sc))


def test_the_semantic_masks(T, ops, oracle, town):
    """the mask instantiations take the path too (their translation unit has work counters of its own, which the hook does not read: the two
    renders are compared without them)"""
    sc = scene(town, 65, 'crowd')
    sc['mask'][:, :, 2] = False
    smap = town['smap']
    ak = actor_keys(smap, B, 65)
    table = sorted(int(k) & 0xffffffff for k in set(ak.flatten().tolist()))
    chans = {k: 1 for k in table}
    chans.update({int(k) & 0xffffffff: 2 for k in smap.face_keys()})
    sd = dev(sc['state'])
    call = lambda: ops.raster_scene_masks(smap, sd, ops.heading_sc(sd[..., 2]), dev(oracle.actor_template(sc['size'])), ak, dev(sc['mask']), dev(sc['cam_xy']),
                                          ops.heading_sc(dev(sc['psi'])), FOV, RES, table, chans, 2).to(torch.uint8)
    m = both(T, call, None)
    assert bool(m[:, :, 0].any()) and bool(m[:, :, 1].any())
