"""The range-scan kernel (csrc/scan.hip) through Simulator.compute_range_scan on the device, against the float64 model of its definition
(tests/range_scan_model.py: brute force over all faces and all entities), and the batch plumbing around it.

The bar: |kernel - model| <= 1e-4 m for both ranges at max_range <= 100 m -- 6 x the largest float32-against-float64 difference of the model itself
(tests/test_range_scan_model.py prints and asserts that table: 1.32e-5 m over 38 400 rays here, 1.7e-5 m in the prototype the bar was set from).
`hit` equals the model's except where the model's two best candidates (the entities' distances, the road range, max_range) lie within that 1e-4 m.
A ray is excepted from the road bar only when the MODEL calls it threshold-sensitive (its float64 road range differs between gap_tolerance x
(1 - 1e-3) and x (1 + 1e-3)); excepted rays are listed and may be at most 0.01 % of the rays of the test."""
import math
import os

import numpy as np
import pytest
import torch

import range_scan_model as rm
from conftest import GOLDEN
from test_range_scan_model import GPU_BAR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXCEPTION_SHARE = 1e-4


@pytest.fixture(scope='module')
def towns():
    import bench
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.mesh import BirdviewMesh
    lanes = [lanelet2.load_lanelet_map(os.path.join(GOLDEN, f'carla_Town0{k}.osm.gz'), origin=(0.0, 0.0)) for k in (1, 2)]
    raw = [bench.load_town01(), bench.load_town02()]
    meshes = [BirdviewMesh(verts=torch.from_numpy(v)[None], faces=torch.from_numpy(f.astype(np.int64))[None], categories=c, colors={}, zs={},
                           vert_category=torch.from_numpy(vc.astype(np.int64))[None]) for v, f, vc, c in raw]
    return lanes, meshes, [(v, f.astype(np.int64)) for v, f, _, _ in raw]


def make_sim(towns, which, A, seed, npc=0, collate=False, edit=None, road=True):
    """a Simulator of len(which) scenes, scene b on town which[b], A exposed agents and `npc` NPCs placed by heuristic_initialize_batch;
    edit(states, present) may move them by hand"""
    from torchdrivesim_amd.behavior import heuristic_initialize_batch
    from torchdrivesim_amd.kinematic import KinematicBicycle
    from torchdrivesim_amd.mesh import BirdviewMesh
    from torchdrivesim_amd.rendering import HipRendererConfig, renderer_from_config
    from torchdrivesim_amd.simulator import NPCController, Simulator, TorchDriveConfig
    from torchdrivesim_amd.utils import Resolution
    lanes, meshes, _ = towns
    B = len(which)
    if not road:
        mesh = BirdviewMesh.empty(batch_size=B).to(DEV)
    elif len(set(which)) == 1 and not collate:
        mesh = meshes[which[0]].expand(B).to(DEV)
    else:
        mesh = BirdviewMesh.collate(meshes).to(DEV)[list(which)]
    # sizes by agent index (the same in every scene): cars, a few long vehicles, some boxes wider than long
    g = np.random.default_rng(seed)
    sizes = np.stack([g.uniform(3.5, 6.0, A + npc), g.uniform(1.6, 2.4, A + npc)], -1)
    sizes[g.random(A + npc) < 0.15] = [0.9, 1.7]
    attr = np.concatenate([sizes, 0.4 * sizes[:, :1]], -1).astype(np.float32)
    attributes, states, placed = heuristic_initialize_batch([lanes[w] for w in which], B, A + npc, seed=seed, device=DEV,
                                                            agent_attributes=torch.from_numpy(attr).to(DEV).expand(B, -1, -1).contiguous())
    assert bool(placed.all())
    states, placed = states.clone(), placed.clone()
    if edit is not None:
        edit(states, placed)
    km = KinematicBicycle()
    km.set_params(lr=attributes[:, :A, 2].contiguous())
    km.set_state(states[:, :A].contiguous())
    ctrl = None
    if npc:
        ctrl = NPCController(npc_size=attributes[:, A:, :2].contiguous(), npc_state=states[:, A:].contiguous(), npc_present_mask=placed[:, A:].contiguous())
    cfg = TorchDriveConfig(renderer=HipRendererConfig())
    renderer = renderer_from_config(cfg.renderer, res=Resolution(64, 64), fov=35.0)
    return Simulator(mesh, km, attributes[:, :A, :2].contiguous(), placed[:, :A].contiguous(), cfg, renderer=renderer, npc_controller=ctrl)


def model_inputs(sim, n_rays, fov):
    """exactly what compute_range_scan hands to the kernel, as numpy arrays"""
    from torchdrivesim_amd import _ops
    st = sim.get_all_agent_state()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1)
    ray_sc = _ops.heading_sc(sim.get_state()[..., 2].unsqueeze(-1) + sim.range_scan_angles(n_rays, fov).to(DEV))
    return boxes.cpu().numpy(), sim._heading_sc().cpu().numpy(), sim.get_all_agent_present_mask().cpu().numpy(), ray_sc.cpu().numpy()


def compare(name, scan, sim, towns, which, n_rays, fov, max_range, gap=0.02, road=True, agents=True):
    """-> (rays, failures, excepted): the kernel's three outputs against the model's, scene by scene"""
    _, _, raw = towns
    boxes, sc, present, ray_sc = model_inputs(sim, n_rays, fov)
    k_agents, k_road, k_hit = scan.agents.cpu().numpy(), scan.road.cpu().numpy(), scan.hit.cpu().numpy()
    A = ray_sc.shape[1]
    assert k_agents.shape == k_road.shape == k_hit.shape == ray_sc.shape[:3] and k_hit.dtype == np.int32 and k_agents.dtype == np.float32
    assert not scan.agents.requires_grad and not scan.road.requires_grad
    failures, excepted = [], []
    worst = dict(agents=0.0, road=0.0)
    for b, w in enumerate(which):
        verts, faces = raw[w] if road else (None, None)
        m = rm.range_scan(verts, faces, boxes[b], sc[b], present[b], ray_sc[b], max_range, gap, with_agents=agents, sensitivity=road)
        d_agents = np.abs(k_agents[b].astype(np.float64) - m['agents'])
        d_road = np.abs(k_road[b].astype(np.float64) - m['road'])
        sensitive = (m['road_lo'] != m['road_hi']) if road else np.zeros_like(d_road, bool)
        worst['agents'] = max(worst['agents'], float(d_agents.max()))
        worst['road'] = max(worst['road'], float(d_road[~sensitive].max()) if (~sensitive).any() else 0.0)
        for a, k in zip(*np.nonzero(d_agents > GPU_BAR)):
            failures.append(f'{name} scene {b} agent {a} ray {k}: agents {k_agents[b, a, k]!r}, model {m["agents"][a, k]!r}')
        for a, k in zip(*np.nonzero(d_road > GPU_BAR)):
            line = f'{name} scene {b} agent {a} ray {k}: road {k_road[b, a, k]!r}, model {m["road"][a, k]!r} ({m["road_lo"][a, k]!r} .. {m["road_hi"][a, k]!r} around the tolerance)' if road else f'{name} scene {b} agent {a} ray {k}: road {k_road[b, a, k]!r} without a mesh'
            (excepted if sensitive[a, k] else failures).append(line)
        # hit: the model's, unless its two best candidates are within the bar of each other (the kernel's ranges may then order them the other way)
        cand = np.concatenate([np.minimum(m['t'], max_range), m['road'][..., None], np.full(m['road'].shape + (1,), float(max_range))], -1)
        two = np.sort(cand, -1)[..., :2]
        clear = (two[..., 1] - two[..., 0] > GPU_BAR) & ~(d_road > GPU_BAR)
        for a, k in zip(*np.nonzero(clear & (k_hit[b] != m['hit']))):
            failures.append(f'{name} scene {b} agent {a} ray {k}: hit {k_hit[b, a, k]}, model {m["hit"][a, k]} (agents {m["agents"][a, k]!r}, road {m["road"][a, k]!r})')
        absent = ~present[b, :A]
        assert (k_agents[b][absent] == np.float32(max_range)).all() and (k_road[b][absent] == np.float32(max_range)).all() and (k_hit[b][absent] == -1).all()
    print(f'{name:34s} rays {k_hit.size:6d}  max |kernel - model|: agents {worst["agents"]:.3e} m, road {worst["road"]:.3e} m, excepted {len(excepted)}, '
          f'mean road {k_road.mean():.2f} m, hits: entity {(k_hit >= 0).mean():.3f} road edge {(k_hit == -2).mean():.3f} none {(k_hit == -1).mean():.3f}')
    return k_hit.size, failures, excepted


# name: (towns of the scenes, A, NPCs, rays, fov, max_range)
CASES = {
    'town01 R=64 2pi': ([0] * 6, 32, 0, 64, 2 * math.pi, 50.0),
    'town02 R=64 2pi range 100': ([1] * 6, 32, 0, 64, 2 * math.pi, 100.0),
    'town01 R=100 pi/2': ([0] * 4, 32, 0, 100, math.pi / 2, 50.0),
    'town02 R=16 2pi': ([1] * 8, 48, 0, 16, 2 * math.pi, 50.0),
    'town01 R=1 2pi': ([0] * 8, 64, 0, 1, 2 * math.pi, 100.0),
    'town02 R=100 2pi npcs': ([1] * 2, 24, 8, 100, 2 * math.pi, 50.0),
    'both R=64 pi/2 npcs': ([0, 1, 1, 0], 12, 4, 64, math.pi / 2, 30.0),
}


def hand_placed(states, present):
    """scene 0: agents outside the grid, off the road and overlapping; an NPC in front of an agent.  scene 1: two agents on the same spot, an
    absent exposed agent and an absent NPC.  (A = 16 exposed agents, 4 NPCs)"""
    dev = states.device
    states[0, 0, :2] = torch.tensor([-500.0, -500.0], device=dev)
    states[0, 1, :2] = torch.tensor([1000.0, 50.0], device=dev)
    states[0, 2, :2] = torch.tensor([60.0, 60.0], device=dev)                  # inside a block of Town01
    states[0, 3, :2] = states[0, 4, :2] + torch.tensor([45.0, 0.0], device=dev)
    states[0, 5, :3] = states[0, 4, :3] + torch.tensor([0.3, 0.2, 0.2], device=dev)
    states[0, 16, :2] = states[0, 6, :2] + torch.tensor([5.0, 0.5], device=dev)
    states[0, 17, :3] = states[0, 7, :3] + torch.tensor([0.0, 0.0, 1.0], device=dev)
    states[1, 1] = states[1, 0]
    present[1, 3] = False
    present[1, 18] = False
    states[1, 19, :2] = states[1, 2, :2] + torch.tensor([-6.0, 1.0], device=dev)


def test_kernel_against_the_float64_model(towns):
    """[the figures of the last run on an MI355X are in DESIGN.md, "K5"]"""
    total, failures, excepted = 0, [], []
    for name, (which, A, npc, R, fov, max_range) in CASES.items():
        sim = make_sim(towns, which, A, seed=len(name) + R, npc=npc)
        scan = sim.compute_range_scan(n_rays=R, max_range=max_range, fov=fov)
        n, f, e = compare(name, scan, sim, towns, which, R, fov, max_range)
        total, failures, excepted = total + n, failures + f, excepted + e
    # by hand
    sim = make_sim(towns, [0, 0], 16, seed=5, npc=4, edit=hand_placed)
    scan = sim.compute_range_scan(n_rays=64, max_range=50.0)
    n, f, e = compare('town01 hand-placed', scan, sim, towns, [0, 0], 64, 2 * math.pi, 50.0)
    total, failures, excepted = total + n, failures + f, excepted + e
    assert bool((scan.road[0, :3] == 0).all()) and bool((scan.hit[0, :3] == -2).all())          # outside the grid and off the road: no road at all
    assert bool((scan.agents[0, 4] == 0).all()) and bool((scan.agents[1, 0] == 0).all()) and bool((scan.hit[1, 0] == 1).all())
    assert bool(scan.agents[0, 6].min() < 6.0) and bool((scan.hit[1] != 18).all()) and bool((scan.hit[1] != 3).all())
    # the parts alone: the other range is max_range
    for kw in (dict(road=False), dict(agents=False)):
        part = sim.compute_range_scan(n_rays=64, max_range=50.0, **kw)
        n, f, e = compare(f'town01 hand-placed {kw}', part, sim, towns, [0, 0], 64, 2 * math.pi, 50.0, road=kw.get('road', True), agents=kw.get('agents', True))
        total, failures, excepted = total + n, failures + f, excepted + e
        same, other = ('agents', 'road') if 'road' in kw else ('road', 'agents')
        assert torch.equal(getattr(part, same), getattr(scan, same)) and bool((getattr(part, other) == 50.0).all())
    # no road mesh at all
    sim = make_sim(towns, [0, 0, 0], 16, seed=6, npc=2, road=False)
    scan = sim.compute_range_scan(n_rays=16, max_range=40.0)
    n, f, e = compare('no road mesh', scan, sim, towns, [0, 0, 0], 16, 2 * math.pi, 40.0, road=False)
    total, failures, excepted = total + n, failures + f, excepted + e
    assert bool((scan.road == 40.0).all()) and bool((scan.hit != -2).all())
    print(f'{total} rays, {len(failures)} beyond the bar of {GPU_BAR} m, {len(excepted)} excepted as threshold-sensitive')
    assert total >= 50000
    assert not failures, f'{len(failures)} of {total} rays miss the model:\n' + '\n'.join(failures[:40])
    assert len(excepted) <= EXCEPTION_SHARE * total, f'{len(excepted)} threshold-sensitive rays of {total} (at most 0.01 %):\n' + '\n'.join(excepted[:40])


def test_identical_boxes_tie_to_the_lowest_index():
    """Entities 1, 2 and 3 are the SAME box, so the kernel's distances to them are the same bits: every ray that meets them must name entity 1 --
    the tie rule itself, which the comparison with the model leaves out (two candidates within the bar).  Seen from outside, from inside, and
    with the lowest of them absent."""
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.simulator import Simulator
    R = 64
    same = [10.0, 0.5, 4.6, 1.9, 0.4]
    boxes = torch.tensor([[[0.0, 0.0, 4.0, 2.0, 0.1], same, same, same, [-10.0, 3.0, 4.0, 2.0, 2.0]],
                          [[10.3, 0.4, 4.0, 2.0, 0.1], same, same, same, [-10.0, 3.0, 4.0, 2.0, 2.0]],
                          [[0.0, 0.0, 4.0, 2.0, 0.1], same, same, same, [-10.0, 3.0, 4.0, 2.0, 2.0]]], device=DEV)
    present = torch.ones(3, 5, dtype=torch.bool, device=DEV)
    present[2, 1] = False
    sc = _ops.heading_sc(boxes[..., 4])
    ray_sc = _ops.heading_sc(boxes[:, :1, 4].unsqueeze(-1) + Simulator.range_scan_angles(R).to(DEV))
    agents, road, hit = _ops.range_scan(None, boxes, sc, present, ray_sc, 1, 50.0, 0.02)
    for b, lowest in ((0, 1), (1, 1), (2, 2)):
        on_them = (hit[b] >= 1) & (hit[b] <= 3)
        assert bool(on_them.any()) and bool((hit[b][on_them] == lowest).all()), (b, hit[b])
    assert bool((hit[1] == 1).all()) and bool((agents[1] == 0).all())             # from inside them: every ray, at 0 m
    assert bool((hit[0] == 4).any()) and bool((road == 50.0).all())


def equal(a, b):
    return torch.equal(a.agents, b.agents) and torch.equal(a.road, b.road) and torch.equal(a.hit, b.hit)


def rows(scan, idx):
    from torchdrivesim_amd.simulator import RangeScan
    return RangeScan(scan.agents[idx], scan.road[idx], scan.hit[idx])


def test_a_batch_on_two_maps_equals_the_single_map_runs(towns):
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.infractions import _static_maps_for
    which = [0, 1] * 4
    sim = make_sim(towns, which, 24, seed=31, npc=3)
    whole = sim.compute_range_scan(n_rays=64, max_range=60.0)
    assert isinstance(_static_maps_for(sim.road_mesh, torch.device(DEV)), _ops.StaticMapSet)
    assert bool((whole.road > 0).float().mean() > 0.9) and bool((whole.hit >= 0).any()) and bool((whole.hit == -2).any())
    for w in (0, 1):
        idx = [b for b in range(len(which)) if which[b] == w]
        part = sim.select_batch_elements(idx, in_place=False)
        assert isinstance(_static_maps_for(part.road_mesh, torch.device(DEV)), _ops.StaticMap)
        assert equal(part.compute_range_scan(n_rays=64, max_range=60.0), rows(whole, idx))
        # ... and the town's own mesh, not padded to the larger one: another grid, the same ranges
        alone = make_sim(towns, [w] * len(idx), 24, seed=31, npc=3)
        alone.kinematic_model.set_state(part.get_state().clone())
        alone.npc_controller.npc_state = part.get_npc_state().clone()
        assert equal(alone.compute_range_scan(n_rays=64, max_range=60.0), rows(whole, idx))


def test_batch_plumbing_reproduces_the_rows_bit_for_bit(towns):
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.parallel import shard_simulator
    which = [0, 1, 1, 0, 0, 1, 0]
    sim = make_sim(towns, which, 20, seed=41, npc=2)
    kw = dict(n_rays=16, max_range=50.0, fov=math.pi / 2)
    whole = sim.compute_range_scan(**kw)
    created = _ops.map_creations
    assert equal(sim.compute_range_scan(**kw), whole) and equal(sim.compute_range_scan(**kw), whole)           # repeated calls
    assert equal(sim.copy().compute_range_scan(**kw), whole)
    idx = [5, 0, 3]
    assert equal(sim.select_batch_elements(idx, in_place=False).compute_range_scan(**kw), rows(whole, idx))
    assert equal(sim[[2]].compute_range_scan(**kw), rows(whole, [2]))
    twice = sim.extend(2, in_place=False).compute_range_scan(**kw)
    assert equal(twice, rows(whole, [b for b in range(len(which)) for _ in range(2)]))
    shards = [shard_simulator(sim, rank, 2).compute_range_scan(**kw) for rank in range(2)]
    assert torch.equal(torch.cat([s.agents for s in shards]), whole.agents) and torch.equal(torch.cat([s.road for s in shards]), whole.road)
    assert torch.equal(torch.cat([s.hit for s in shards]), whole.hit)
    assert _ops.map_creations == created, 'a batch operation or a later call created a device map'


def test_map_creations_do_not_move_after_the_first_call(towns):
    from torchdrivesim_amd import _ops
    sim = make_sim(towns, [1] * 3, 8, seed=51)
    sim.compute_range_scan(n_rays=8)
    created = _ops.map_creations
    sim.compute_offroad()                                  # the same cached map
    for R in (8, 64):
        sim.compute_range_scan(n_rays=R)
    assert _ops.map_creations == created


def test_a_captured_step_and_scan_replays_the_eager_bits(towns):
    sim = make_sim(towns, [0, 1] * 8, 32, seed=61, npc=2)
    ref = make_sim(towns, [0, 1] * 8, 32, seed=61, npc=2)
    B, A = 16, 32
    g0 = torch.Generator(device='cpu').manual_seed(3)
    actions = (torch.rand(4, B, A, 2, generator=g0) * 2 - 1).to(DEV)
    state = sim.get_state().clone()
    action = actions[0].clone()
    sim.kinematic_model.set_state(state)

    def step():
        sim.kinematic_model.set_state(state)
        sim.step(action)
        scan = sim.compute_range_scan(n_rays=64, max_range=50.0)
        return scan, sim.get_state()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()                                          # builds the device maps and their set
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        scan, new = step()
        state_next = new.clone()
    for i in range(4):
        ref.kinematic_model.set_state(state.clone())
        ref.step(actions[i])
        want = ref.compute_range_scan(n_rays=64, max_range=50.0)
        action.copy_(actions[i])
        g.replay()
        torch.cuda.synchronize()
        assert equal(scan, want) and torch.equal(new, ref.get_state())
        assert bool((scan.road < 50.0).any()) and bool((scan.hit >= 0).any())
        state.copy_(state_next)


def test_ray_offsets_built_on_the_device_are_the_hosts_bits():
    """compute_range_scan builds the offsets on the device (nothing crosses from the host: a fresh copy of a simulator can be captured too);
    they are the bits of the host's formula"""
    from torchdrivesim_amd.simulator import Simulator
    for R, fov in ((1, 2 * math.pi), (16, 2 * math.pi), (64, math.pi / 2), (100, 1.0), (4097, 2 * math.pi), (65536, 3.0)):
        assert torch.equal(Simulator.range_scan_angles(R, fov, device=DEV).cpu(), Simulator.range_scan_angles(R, fov)), (R, fov)
