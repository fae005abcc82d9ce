"""Semantic bird's-eye masks on an MI355X (Simulator.render_semantic / render_egocentric_semantic -> tds_raster_scene_masks): bit for bit
against the CPU oracle rendering each channel's categories white over a black scene, consistent with the colour image of the same call,
`out=` and graph capture, and the documented refusal of scenes with more than 15 keys."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_simulator import make_sim, two_towns

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TYPES = ['vehicle', 'bicycle', 'pedestrian']
SIZES = np.array([[4.5, 1.8], [1.8, 0.7], [0.7, 0.7]], np.float32)
TOP, BOTTOM = 1.0, 100.0          # levels of the recoloured reference: a channel's categories white on top, everything else black below


def unpack(words, res):
    from torchdrivesim_amd.rendering import unpack_mask_bits
    return unpack_mask_bits(words, res)


def both_modes(sim, *args, **kw):
    """(bool masks, packed masks unpacked) of one render_semantic call"""
    from torchdrivesim_amd.utils import Resolution
    res = kw['res']
    kw['res'] = Resolution(res, res)
    a = sim.render_semantic(*args, **kw)
    b = sim.render_semantic(*args, packed=True, **kw)
    assert a.dtype == torch.bool and b.dtype == torch.int32 and b.shape[-2:] == ((res + 31) // 32, res)
    return a.cpu().numpy(), unpack(b, res).cpu().numpy()


def fuzz_sim(order, A, seed):
    """a batch of Town01 / Town02 scenes (order: 0 = Town01, 1 = Town02) with A agents of three types near the roads"""
    road, pair = two_towns(order)
    rng = np.random.default_rng(seed)
    B = len(order)
    state = np.zeros((B, A, 4), np.float32)
    for b, t in enumerate(order):
        v = pair.verts[t].numpy()
        f = pair.faces[t].numpy()
        f = f[(f != 0).any(1)]
        centre = v[f[rng.integers(0, len(f), A)]].mean(1)[:, :2]
        state[b, :, :2] = centre + rng.uniform(-4, 4, (A, 2))
        state[b, :, 2] = rng.uniform(-np.pi, np.pi, A)
    types = rng.integers(0, 3, (B, A))
    types[:, :3] = [0, 1, 2]                                            # every type in every scene
    present = rng.random((B, A)) < 0.9
    sim = make_sim(state, SIZES[types], present, road, agent_types=torch.from_numpy(types).to(DEV), agent_type_names=TYPES)
    return sim, pair, types, present


def recoloured(cats, chan):
    colors = {c: ((255, 255, 255) if c in chan else (0, 0, 0)) for c in cats}
    levels = {c: (TOP if c in chan else BOTTOM) for c in cats}
    return colors, levels


def oracle_masks(oracle, sim, pair, order, types, present, cxy, csc, rmask, fov, res, channels):
    """B x Nc x C x res x res: per channel, the oracle's image of the scene recoloured (render_scenes) > 0"""
    from oracle.oracle import DEFAULT_COLORS, DEFAULT_LEVELS
    cats = sorted(set(DEFAULT_COLORS) & set(DEFAULT_LEVELS))
    B, Nc = cxy.shape[:2]
    state = sim.get_all_agent_state().detach().cpu().numpy()
    size = sim.get_all_agent_size().detach().cpu().numpy()
    asc = sim._heading_sc().detach().cpu().numpy()
    mask = present[:, None, :] & rmask
    out = np.zeros((B, Nc, len(channels), res, res), bool)
    for t in sorted(set(order)):
        bs = [b for b in range(B) if order[b] == t]
        for c, chan in enumerate(channels):
            colors, levels = recoloured(cats, chan)
            sv, sa, sf = oracle.static_mesh_arrays(pair.verts[t].numpy(), pair.faces[t].numpy(), pair.vert_category[t].numpy(),
                                                   list(pair.categories), colors=colors, levels=levels)
            tn = types[bs]
            al = np.stack([np.vectorize(lambda i: levels[TYPES[i]])(tn), np.full(tn.shape, levels['direction'])], -1).astype(np.float32)
            ac = np.stack([np.array([colors[TYPES[i]] for i in tn.reshape(-1)], np.float32).reshape(tn.shape + (3,)),
                           np.broadcast_to(np.array(colors['direction'], np.float32), tn.shape + (3,))], -2) / np.float32(255.0)
            ref = oracle.render_scenes(state[bs], size[bs], mask[bs], cxy[bs], csc[bs], sv, sa, sf, fov, res, agent_sc=asc[bs],
                                       actor_levels=al, actor_colors=ac.astype(np.float32))
            out[bs, :, c] = ref.max(axis=2) > 0
    return out


# resolution -> cameras (about 2 000 in all): the split form up to 216 px, the fused persistent kernel above, odd sizes on the one-pixel path
RES_CAMS = ((4, 400), (31, 400), (64, 300), (100, 240), (128, 240), (160, 160), (200, 96), (216, 96), (256, 48), (512, 16))


def test_masks_equal_the_oracle_on_fuzzed_town_cameras(oracle):
    """Town01 and Town02 in one batch, three agent types (seven keys: the 8-wave kernel at 256 px), a rendering mask, masked agents; the
    default channels and two unions; both output modes"""
    order = (0, 1, 0, 1)
    sim, pair, types, present = fuzz_sim(order, 24, 5)
    chans = sim.semantic_channels()
    assert chans == ['road', 'right_lane', 'left_lane', 'pedestrian', 'bicycle', 'vehicle', 'direction']
    channels = [(c,) for c in chans] + [('road', 'left_lane', 'right_lane'), ('vehicle', 'bicycle', 'pedestrian', 'direction')]
    rng = np.random.default_rng(11)
    B, A = len(order), 24
    total = 0
    state = sim.get_all_agent_state().detach().cpu().numpy()
    for res, cams in RES_CAMS:
        Nc = cams // B
        fov = float(rng.uniform(20, 70))
        cxy = (state[:, rng.integers(0, A, Nc), :2] + rng.uniform(-6, 6, (B, Nc, 2))).astype(np.float32)
        psi = torch.from_numpy(rng.uniform(-np.pi, np.pi, (B, Nc, 1)).astype(np.float32)).to(DEV)
        csc = torch.cat([torch.sin(psi), torch.cos(psi)], -1).cpu().numpy()
        rmask = rng.random((B, Nc, A)) < 0.8
        m8, mb = both_modes(sim, torch.from_numpy(cxy).to(DEV), psi, channels=channels, res=res, fov=fov, rendering_mask=torch.from_numpy(rmask).to(DEV))
        ref = oracle_masks(oracle, sim, pair, order, types, present, cxy, csc, rmask, fov, res, channels)
        for c, chan in enumerate(channels):
            np.testing.assert_array_equal(m8[:, :, c], ref[:, :, c], err_msg=f'res {res} channel {chan} (uint8 masks)')
            np.testing.assert_array_equal(mb[:, :, c], ref[:, :, c], err_msg=f'res {res} channel {chan} (packed masks)')
        assert ref[:, :, 0].any() and (res < 64 or ref[:, :, 3:7].any())
        total += B * Nc
    assert total >= 1900


def test_masks_equal_the_oracle_on_the_golden_scenes(oracle):
    """G5 (town01_128, town01_64_lh) through render_egocentric_semantic"""
    import json
    from test_gpu_simulator import town_mesh
    g = load_golden('g45_mesh_preraster.npz')
    meta = {m['name']: m for m in json.loads(str(g['g5_meta']))}
    for name in ('town01_128', 'town01_64_lh'):
        m = meta[name]
        st, sz, pr = g[f'g5_{name}_state'], g[f'g5_{name}_size'], g[f'g5_{name}_present']
        B, A = st.shape[:2]
        road, t = town_mesh(B)
        sim = make_sim(st, sz, pr, road)
        sim.cfg.left_handed_coordinates = m['left_handed']
        from torchdrivesim_amd.utils import Resolution
        chans = sim.semantic_channels()
        res = m['res']
        a = sim.render_egocentric_semantic(res=Resolution(res, res), fov=m['fov']).cpu().numpy()
        b = unpack(sim.render_egocentric_semantic(res=Resolution(res, res), fov=m['fov'], packed=True), res).cpu().numpy()
        s = sim.get_state()
        sc = torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1).cpu().numpy()
        mask = np.ascontiguousarray(np.broadcast_to(pr[:, None, :], (B, A, A)))
        cats = [str(c) for c in t['categories']]
        from oracle.oracle import DEFAULT_COLORS, DEFAULT_LEVELS
        for c, chan in enumerate(chans):
            colors, levels = recoloured(set(DEFAULT_COLORS) & set(DEFAULT_LEVELS), (chan,))
            sv, sa, sf = oracle.static_mesh_arrays(t['verts'], t['faces'], t['vert_category'], cats, colors=colors, levels=levels)
            al = np.broadcast_to(np.array([levels['vehicle'], levels['direction']], np.float32), (B, A, 2))
            ac = np.broadcast_to(np.array([colors['vehicle'], colors['direction']], np.float32) / np.float32(255.0), (B, A, 2, 3))
            ref = oracle.render_scenes(st, sz, mask, st[..., :2].copy(), sc, sv, sa, sf, m['fov'], res, agent_sc=sc, actor_levels=al,
                                       actor_colors=ac).max(axis=2) > 0
            np.testing.assert_array_equal(a[:, :, c], ref, err_msg=f'{name} {chan}')
            np.testing.assert_array_equal(b[:, :, c], ref, err_msg=f'{name} {chan} packed')


def test_traffic_controls_and_waypoints_agree_with_the_oracle_image(oracle):
    """G9 (stop lines, yield lines, lights by state) and G11 (waypoint discs, masked waypoints): the colour image of the same call is the
    oracle's drawing of the reference's explicit mesh (as in test_gpu_simulator.py), and the masks resolved by key give exactly that image;
    the split form (96, 128 px) and the fused kernel (256, 320 px: two strips); both output modes"""
    from test_waypoints import sim_with_goals
    from torchdrivesim_amd.traffic_controls import StopSignControl, TrafficLightControl, YieldControl
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.utils import Resolution
    g = load_golden('g9_traffic_mesh.npz')
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    B, A = g['state'].shape[:2]
    road = BirdviewMesh(verts=d(g['bg_verts'])[None], faces=d(g['bg_faces'].astype(np.int64))[None], categories=['right_lane', 'left_lane', 'road'],
                        colors={}, zs={}, vert_category=d(g['bg_vert_category'].astype(np.int64))[None]).expand(B)
    tl = TrafficLightControl(d(g['tl_pos']), mask=d(g['tl_mask']))
    tl.set_state(d(g['tl_state']))
    controls = dict(stop_sign=StopSignControl(d(g['ss_pos'])), traffic_light=tl, yield_sign=YieldControl(d(g['ys_pos'])))
    sim = make_sim(g['state'], g['size'], g['present'], road, traffic_controls=controls)
    chans = sim.semantic_channels()
    assert {'stop_sign', 'yield_sign', 'traffic_light_red', 'traffic_light_green'} <= set(chans)
    s = sim.get_state()
    cam_sc = torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1)
    for res, fov in ((128, 35.0), (256, 60.0)):
        ref = oracle.render_rgb_mesh(g['rgb_verts'], g['rgb_attrs'], g['rgb_faces'], s[..., :2].reshape(-1, 2).cpu().numpy(),
                                     cam_sc.reshape(-1, 2).cpu().numpy(), 2.0 / fov, res)
        ref = torch.from_numpy(np.transpose(ref, (0, 3, 1, 2)).reshape(B, A, 3, res, res)).to(DEV)
        masks = sim.render_egocentric_semantic(res=Resolution(res, res), fov=fov)
        bits = unpack(sim.render_egocentric_semantic(res=Resolution(res, res), fov=fov, packed=True), res)
        assert torch.equal(masks, bits)
        assert torch.equal(sim.render_egocentric(res=Resolution(res, res), fov=fov), ref)
        assert torch.equal(winner_image(sim, masks, chans).to(torch.float32), ref)
        lights = [i for i, c in enumerate(chans) if c.startswith('traffic_light')]
        assert masks[:, :, lights].any()
        # coverage, not visibility: the road channel holds pixels the image shows in other colours
        road_px = (ref == torch.tensor([155.0, 155.0, 155.0], device=DEV).view(1, 1, 3, 1, 1)).all(2)
        assert (masks[:, :, chans.index('road')] & ~road_px).any()
    # waypoint goals: the fused path's image is the oracle's drawing of generate()'s mesh (test_waypoint_goals_are_drawn_by_the_fused_path)
    g = load_golden('g11_waypoints.npz')
    sim = sim_with_goals(g, device=DEV)
    chans = sim.semantic_channels()
    assert 'goal_waypoint' in chans
    s = sim.get_state()
    B, A = s.shape[:2]
    mask = sim.get_present_mask()[:, None].expand(B, A, A)
    cam_sc = torch.stack([torch.sin(s[..., 2]), torch.cos(s[..., 2])], -1)
    for count, res, fov in ((2, 96, 35.0), (3, 320, 60.0)):
        rgb = sim.birdview_mesh_generator.generate(A, agent_state=s[:, None].expand(-1, A, -1, -1), present_mask=mask,
                                                   waypoints=sim.get_waypoints(count), waypoints_rendering_mask=sim.get_waypoints_mask(count))
        ref = oracle.render_rgb_mesh(rgb.verts.cpu().numpy(), rgb.attrs.cpu().numpy(), rgb.faces.cpu().numpy().astype(np.int32),
                                     s[..., :2].reshape(-1, 2).cpu().numpy(), cam_sc.reshape(-1, 2).cpu().numpy(), 2.0 / fov, res)
        ref = torch.from_numpy(np.transpose(ref, (0, 3, 1, 2)).reshape(B, A, 3, res, res)).to(DEV)
        masks = sim.render_egocentric_semantic(res=Resolution(res, res), fov=fov, n_subsequent_waypoints=count)
        bits = unpack(sim.render_egocentric_semantic(res=Resolution(res, res), fov=fov, n_subsequent_waypoints=count, packed=True), res)
        assert torch.equal(masks, bits)
        assert torch.equal(sim.render_egocentric(res=Resolution(res, res), fov=fov, n_subsequent_waypoints=count), ref)
        assert torch.equal(winner_image(sim, masks, chans).to(torch.float32), ref)
        assert int(masks[:, :, chans.index('goal_waypoint')].sum()) > 50


def winner_image(sim, masks, chans):
    """the colour the RGB path paints where a channel is set: that of the highest key among the set channels (ascending key = painter order)"""
    keys = sim._category_keys(sim._scene())
    kv = torch.tensor([keys[c] for c in chans], dtype=torch.int64, device=masks.device)
    k = torch.where(masks, kv.view(1, 1, -1, 1, 1), torch.zeros((), dtype=torch.int64, device=masks.device)).amax(dim=2)
    rgb = torch.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], dim=2)
    return rgb


@pytest.mark.parametrize('order', [(0, 0), (0, 1, 1, 0)])
def test_masks_agree_with_the_colour_image(order):
    """one channel per key: the colour image equals, at every pixel, the colour of the highest key whose channel is set (background where
    none is) -- float32 and uint8, one map and a mixed Town01 / Town02 batch"""
    from torchdrivesim_amd.utils import Resolution
    sim, _, _, _ = fuzz_sim(order, 16, 3)
    chans = sim.semantic_channels()
    for res in (64, 128, 256):
        masks = sim.render_egocentric_semantic(res=Resolution(res, res), fov=40.0)
        want = winner_image(sim, masks, chans)
        sim.renderer.cfg.out_dtype = 'float32'
        img = sim.render_egocentric(res=Resolution(res, res), fov=40.0)
        assert torch.equal(img, want.to(torch.float32))
        sim.renderer.cfg.out_dtype = 'uint8'
        img8 = sim.render_egocentric(res=Resolution(res, res), fov=40.0)
        sim.renderer.cfg.out_dtype = 'float32'
        assert torch.equal(img8, want.to(torch.uint8))
        assert masks[:, :, 0].any() and masks[:, :, -2].any()


def test_out_is_honoured_and_a_captured_call_replays_the_same_bytes():
    from torchdrivesim_amd.utils import Resolution
    sim, _, _, _ = fuzz_sim((0, 1), 12, 9)
    res = Resolution(128, 128)
    C = len(sim.semantic_channels())
    eager = sim.render_egocentric_semantic(res=res, fov=40.0)
    eager_bits = sim.render_egocentric_semantic(res=res, fov=40.0, packed=True)
    out = torch.ones((2, 12, C, 128, 128), dtype=torch.bool, device=DEV)
    r = sim.render_egocentric_semantic(res=res, fov=40.0, out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(out, eager)
    out_bits = torch.full((2, 12, C, 4, 128), -1, dtype=torch.int32, device=DEV)
    assert sim.render_egocentric_semantic(res=res, fov=40.0, packed=True, out=out_bits).data_ptr() == out_bits.data_ptr()
    assert torch.equal(out_bits, eager_bits)
    with pytest.raises(RuntimeError, match='`out`'):
        sim.render_egocentric_semantic(res=res, fov=40.0, out=torch.zeros((2, 12, C, 128, 127), dtype=torch.bool, device=DEV))
    # graph capture: warm-up on a side stream, capture, replay after the output was cleared
    cap = torch.zeros_like(out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sim.render_egocentric_semantic(res=res, fov=40.0, out=cap)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sim.render_egocentric_semantic(res=res, fov=40.0, out=cap)
    cap.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager)


def test_more_than_15_keys_is_the_documented_error():
    from torchdrivesim_amd import _native, _ops
    n = 20
    verts = torch.tensor([[float(i), 0.0] for i in range(n)] + [[float(i), 1.0] for i in range(n)])
    faces = torch.tensor([[i, i + 1, n + i] for i in range(n - 1)], dtype=torch.int64)
    smap = _ops.StaticMap(verts, faces, np.full(n - 1, 15.0, np.float32), np.arange(1, n, dtype=np.uint32) * 1000, [15.0, 4.0, 2.0], device=DEV)
    cam_xy = torch.zeros((1, 2, 2), device=DEV)
    cam_sc = torch.tensor([[[0.0, 1.0], [1.0, 0.0]]], device=DEV)
    empty = torch.zeros((1, 0, 4), device=DEV)
    with pytest.raises(_native.TdsError) as e:
        _ops.raster_scene_masks(smap, empty, torch.zeros((1, 0, 2), device=DEV), torch.zeros((1, 0, 7, 2), device=DEV),
                                torch.zeros((1, 0, 2), dtype=torch.int32, device=DEV), torch.zeros((1, 2, 0), dtype=torch.bool, device=DEV),
                                cam_xy, cam_sc, 30.0, 64, [], {k: 1 for k in smap.face_keys()}, 1)
    assert e.value.code == _native.E_LIMIT and 'bit-plane' in str(e.value)
    torch.cuda.synchronize()
    # the device is fine: a scene within the limit renders
    few = _ops.StaticMap(verts, faces[:3], np.full(3, 15.0, np.float32), np.array([1000, 2000, 3000], np.uint32), [15.0, 4.0, 2.0], device=DEV)
    m = _ops.raster_scene_masks(few, empty, torch.zeros((1, 0, 2), device=DEV), torch.zeros((1, 0, 7, 2), device=DEV),
                                torch.zeros((1, 0, 2), dtype=torch.int32, device=DEV), torch.zeros((1, 2, 0), dtype=torch.bool, device=DEV),
                                cam_xy, cam_sc, 30.0, 64, [], {k: 1 for k in few.face_keys()}, 1)
    torch.cuda.synchronize()
    assert m.shape == (1, 2, 1, 64, 64) and m.any()
