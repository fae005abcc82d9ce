"""The on-lane spawn kernel (csrc/spawn.hip) on the device: against the CPU model (tests/spawn_model.py, itself pinned to the reference's
heuristic_initialize by G16), through `heuristic_initialize_batch` and through the raw `_ops.spawn_on_lanes`; what a user relies on (no
overlaps, no wrong-way agents); the identity of a scene in the random stream; failure; capture into a graph."""
import os

import numpy as np
import pytest
import torch

import spawn_model as sm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GAP = (1.0, 0.2)


@pytest.fixture(scope='module')
def towns():
    from torchdrivesim_amd import lanelet2
    maps = [lanelet2.load_lanelet_map(os.path.join(GOLDEN, f'carla_Town0{k}.osm.gz'), origin=(0.0, 0.0)) for k in (1, 2)]
    return maps, [sm.Lanes(lanelet2.lane_table(m)) for m in maps]


def short_map(length=30.0):
    from torchdrivesim_amd import lanelet2
    return lanelet2.LaneletMap([], np.zeros((0, 3)), [lanelet2.make_lanelet(1, [(0.0, 1.75), (length, 1.75)], [(0.0, -1.75), (length, -1.75)])])


def mixed_attributes(B, A, seed):
    """per-agent sizes: cars, a few long vehicles, and some boxes WIDER than long (the disc chain then runs across the heading)"""
    g = np.random.default_rng(seed)
    at = np.empty((B, A, 3), np.float32)
    at[..., 0] = g.uniform(3.5, 6.0, (B, A))
    at[..., 1] = g.uniform(1.6, 2.4, (B, A))
    wide = g.random((B, A)) < 0.15
    at[..., 0][wide], at[..., 1][wide] = g.uniform(0.6, 1.0, int(wide.sum())), g.uniform(1.2, 2.0, int(wide.sum()))
    at[:, 0, 0], at[:, 0, 1] = 0.8, 1.9                      # every scene starts with one
    at[..., 2] = at[..., 0] * 0.4
    return at


def assert_within_one_ulp(got, want, what):
    ok = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    assert ok.all(), f'{what}: {int((~ok).sum())} values further than one float32 ulp from the model'


# name: (maps per scene as indices into towns, A, per-agent attributes, occupied boxes per scene); B = 16 / 12 / 12 / 4 / 3 scenes -- 47 in all,
# a second or two of model time
CASES = {
    'town01_a64': ([0] * 16, 64, False, 0),
    'town02_a64_attributes': ([1] * 12, 64, True, 0),
    'both_a64_occupied': ([0, 1] * 6, 64, False, 7),
    'town01_a256': ([0] * 4, 256, False, 0),
    'both_a256_attributes_occupied': ([1, 0, 1], 256, True, 9),
}


@pytest.mark.parametrize('case', list(CASES))
def test_kernel_equals_the_model(case, towns, oracle):
    """x, y, speed, [sin, cos], placed and attempts exactly; psi within one float32 ulp (a float64 atan2 rounded once)"""
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    from torchdrivesim_amd.infractions import LANELET_TAGS_TO_EXCLUDE
    maps, lanes = towns
    which, A, own_attributes, M = CASES[case]
    B, seed = len(which), 0xC0FFEE ^ len(case)
    scene_ids = torch.arange(1000, 1000 + B, device=DEV) * 7
    attributes = mixed_attributes(B, A, 5) if own_attributes else np.stack([sm.default_attributes(A)] * B)
    attr_d = torch.from_numpy(attributes).to(DEV)
    occupied = occupied_mask = occ_sc = None
    if M:
        # boxes standing on the lanes already: the first agents of another draw, one of them masked out, one wider than long
        _, st, _ = heuristic_initialize_batch([maps[w] for w in which], B, M, seed=seed + 1, device=DEV)
        occupied = torch.cat([st[..., :2], torch.tensor([4.97, 2.04], device=DEV).expand(B, M, 2), st[..., 2:3]], -1).contiguous()
        occupied[:, 1, 2:4] = torch.tensor([1.0, 2.5], device=DEV)
        occupied_mask = torch.ones(B, M, dtype=torch.bool, device=DEV)
        occupied_mask[:, 2] = False
        inflated = occupied.clone()
        inflated[..., 2] += GAP[0]
        inflated[..., 3] += GAP[1]
        occ_sc = _ops.metric_sc(inflated, 'discs')
    uniq = sorted(set(which))
    lane_set = _ops.LaneTableSet([maps[u].table(DEV, LANELET_TAGS_TO_EXCLUDE) for u in uniq],
                                 None if len(uniq) == 1 else [uniq.index(w) for w in which])
    state, sc, placed, attempts = _ops.spawn_on_lanes(lane_set, scene_ids, attr_d, seed, 0, 10, GAP, 500, occupied, occ_sc, occupied_mask)
    at2, st2, pl2 = heuristic_initialize_batch([maps[w] for w in which], B, A, seed=seed, scene_ids=scene_ids, agent_attributes=attr_d if own_attributes else None,
                                               occupied=occupied, occupied_mask=occupied_mask, on_failure='mask', device=DEV)
    assert torch.equal(st2, state) and torch.equal(pl2, placed) and torch.equal(at2, attr_d)
    state, sc, placed, attempts = state.cpu().numpy(), sc.cpu().numpy(), placed.cpu().numpy(), attempts.cpu().numpy()
    assert placed.all()
    for b in range(B):
        occ = occ_s = None
        if M:
            keep = occupied_mask[b].cpu().numpy()
            occ, occ_s = occupied[b].cpu().numpy()[keep], occ_sc[b].cpu().numpy()[keep]
        w_state, w_sc, w_placed, w_attempts = sm.spawn_scene(oracle, lanes[which[b]], seed, int(scene_ids[b]), attributes[b], 0, 10, 500, GAP, occ, occ_s)
        assert np.array_equal(placed[b], w_placed) and np.array_equal(attempts[b], w_attempts), f'scene {b}: other candidates were taken'
        assert np.array_equal(state[b][:, [0, 1, 3]].view(np.uint32), w_state[:, [0, 1, 3]].view(np.uint32)), f'scene {b}: x, y or speed differ'
        assert np.array_equal(sc[b].view(np.uint32), w_sc.view(np.uint32)), f'scene {b}: [sin, cos] differ'
        assert_within_one_ulp(state[b][:, 2], w_state[:, 2], f'scene {b}: psi')
    assert (attempts > 1).mean() > 0.1                       # rejection happened


def test_nothing_overlaps_and_nobody_drives_the_wrong_way(towns, oracle):
    import bench
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import Simulator, TorchDriveConfig, CollisionMetric
    from torchdrivesim_amd.utils import Resolution
    maps, _ = towns
    B, A, M = 32, 64, 4
    which = [b % 2 for b in range(B)]
    _, st, _ = heuristic_initialize_batch([maps[w] for w in which], B, M, seed=3, device=DEV)
    occupied = torch.cat([st[..., :2], torch.tensor([4.97, 2.04], device=DEV).expand(B, M, 2), st[..., 2:3]], -1).contiguous()
    attributes, states, placed = heuristic_initialize_batch([maps[w] for w in which], B, A, seed=4, occupied=occupied, device=DEV)
    assert bool(placed.all())
    # every pair of placed agents, the second one grown by the gap, and every (agent, occupied) pair: no disc value above 0
    s, at = states.cpu().numpy(), attributes.cpu().numpy()
    gap = np.array([GAP[0], GAP[1]], np.float32)
    boxes = np.concatenate([s[..., :2], at[..., :2], s[..., 2:3]], -1)
    grown = np.concatenate([s[..., :2], at[..., :2] + gap, s[..., 2:3]], -1)
    occ = occupied.cpu().numpy()
    occ_grown = np.concatenate([occ[..., :2], occ[..., 2:4] + gap, occ[..., 4:5]], -1)
    i, j = np.triu_indices(A, 1)
    assert not (oracle.discs_pairs(np.ascontiguousarray(boxes[:, j]), np.ascontiguousarray(grown[:, i])) > 0).any()
    bi, oi = np.repeat(np.arange(A), M), np.tile(np.arange(M), A)
    assert not (oracle.discs_pairs(np.ascontiguousarray(boxes[:, bi]), np.ascontiguousarray(occ_grown[:, oi])) > 0).any()
    # a Simulator built from the output
    verts, faces, vcat, cats = bench.load_town01()
    road = BirdviewMesh(verts=torch.from_numpy(verts)[None], faces=torch.from_numpy(faces.astype(np.int64))[None], categories=cats, colors={}, zs={},
                        vert_category=torch.from_numpy(vcat.astype(np.int64))[None]).expand(B).to(DEV)
    km = KinematicBicycle()
    km.set_params(lr=attributes[..., 2].contiguous())
    km.set_state(states)
    cfg = TorchDriveConfig(collision_metric=CollisionMetric.discs, renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    sim = Simulator(road, km, attributes[..., :2].contiguous(), placed, cfg, renderer=renderer, lanelet_map=[maps[w] for w in which])
    assert not bool(sim.compute_collision().any())
    assert not bool(sim.compute_wrong_way().any())


def test_a_scene_is_identified_by_its_id_not_by_its_batch(towns):
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    from torchdrivesim_amd.parallel import scene_shard
    maps, _ = towns
    B, A = 64, 64
    which = [maps[b % 2] for b in range(B)]
    whole = heuristic_initialize_batch(which, B, A, seed=11, device=DEV)
    again = heuristic_initialize_batch(which, B, A, seed=11, device=DEV)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    other = heuristic_initialize_batch(which, B, A, seed=12, device=DEV)
    assert not torch.equal(whole[1], other[1])
    k, n = 21, 9
    part = heuristic_initialize_batch(which[k:k + n], n, A, seed=11, scene_ids=torch.arange(k, k + n, device=DEV), device=DEV)
    assert torch.equal(part[1], whole[1][k:k + n]) and torch.equal(part[2], whole[2][k:k + n])
    halves = []
    for rank in range(2):
        a, b = scene_shard(B, rank, 2)
        halves.append(heuristic_initialize_batch(which[a:b], b - a, A, seed=11, scene_ids=torch.arange(a, b, device=DEV), device=DEV))
    assert torch.equal(torch.cat([h[1] for h in halves]), whole[1]) and torch.equal(torch.cat([h[2] for h in halves]), whole[2])
    # one map for all scenes == a list that repeats it
    one = heuristic_initialize_batch(maps[0], 8, A, seed=11, device=DEV)
    listed = heuristic_initialize_batch([maps[0]] * 8, 8, A, seed=11, device=DEV)
    assert torch.equal(one[1], listed[1])
    # the reference's call: one scene, its shapes
    from torchdrivesim_amd.behavior import heuristic_initialize
    at, st = heuristic_initialize(maps[0], 16, seed=11, device=DEV)
    assert tuple(at.shape) == (1, 16, 3) and tuple(st.shape) == (1, 16, 4) and torch.equal(st[0], whole[1][0, :16])
    assert torch.allclose(at[0, 0].cpu(), torch.tensor([4.97, 2.04, 1.96]))
    assert bool(((st[..., 3] >= 0) & (st[..., 3] < 10)).all())


def test_a_scene_without_room_fails_alone(towns, oracle):
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.behavior import InitializationFailedError, heuristic_initialize, heuristic_initialize_batch
    maps, _ = towns
    short = short_map(30.0)
    A = 12
    which = [maps[0], short, maps[1], None]
    at, st, placed = heuristic_initialize_batch(which, 4, A, num_attempts_per_agent=50, seed=5, on_failure='mask', device=DEV)
    p = placed.cpu().numpy()
    assert p[0].all() and p[2].all() and not p[3].any()
    n = int(p[1].sum())
    assert 2 <= n <= 5 and p[1, :n].all() and not p[1, n:].any()          # 30 m of lane hold five 4.97 m cars with 1 m between them at most
    assert not st[1, n:].any() and not st[3].any() and bool(st[1, :n, 0].gt(0).all())
    want = sm.spawn_scene(oracle, sm.Lanes(lanelet2.lane_table(short)), 5, 1, sm.default_attributes(A), 0, 10, 50, GAP)
    assert np.array_equal(want[2], p[1]) and np.array_equal(want[0][:, [0, 1, 3]], st[1].cpu().numpy()[:, [0, 1, 3]])
    with pytest.raises(InitializationFailedError, match=f'scene 1: agent {n}'):
        heuristic_initialize_batch(which[:3], 3, A, num_attempts_per_agent=50, seed=5, device=DEV)
    with pytest.raises(InitializationFailedError):
        heuristic_initialize(short, A, num_attempts_per_agent=50, seed=5, device=DEV)
    # the scenes beside it are those of a batch without it
    alone = heuristic_initialize_batch([maps[0], maps[1]], 2, A, num_attempts_per_agent=50, seed=5, scene_ids=torch.tensor([0, 2], device=DEV), device=DEV)
    assert torch.equal(alone[1], st[[0, 2]])


def test_a_captured_reset_replays_the_eager_one(towns):
    """on_failure='mask' neither allocates outside torch's allocator nor synchronises: the call is a graph node like every per-step call"""
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    maps, _ = towns
    B, A = 32, 64
    which = [maps[b % 2] for b in range(B)]
    scene_ids = torch.arange(B, device=DEV)
    call = lambda: heuristic_initialize_batch(which, B, A, seed=77, scene_ids=scene_ids, on_failure='mask', device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                               # builds the lane tables and their set
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        at, st, placed = call()
    for first in (0, 500):
        scene_ids.copy_(torch.arange(first, first + B, device=DEV))
        want = call()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(at, want[0]) and torch.equal(st, want[1]) and torch.equal(placed, want[2]) and bool(placed.all())
