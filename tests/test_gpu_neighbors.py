"""The neighbour kernel (csrc/neighbors.hip) on the device against the binary32 model of its definition (tests/neighbors_model.py): features and
index BIT FOR BIT, no row excepted -- through the entry point on hand-made and random scenes, at the wave and stride boundaries and at the entity
limit, with a `visible` mask, through Simulator.compute_neighbors and its batch plumbing, and captured into a graph."""
import math
import os

import numpy as np
import pytest
import torch

import neighbors_model as nm
from conftest import GOLDEN
from test_gpu_range_scan import make_sim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def run(s, A, K, max_distance, visible=None):
    """_ops.neighbors on the scenes of a model generator -> numpy features, index"""
    from torchdrivesim_amd import _ops
    t = {k: torch.from_numpy(v).to(DEV) for k, v in s.items()}
    vis = None if visible is None else torch.from_numpy(visible).to(DEV)
    features, index = _ops.neighbors(t['boxes'], t['sc'], t['speed'], t['present'], A, K, max_distance, visible=vis)
    assert features.dtype == torch.float32 and index.dtype == torch.int32 and not features.requires_grad
    return features.cpu().numpy(), index.cpu().numpy()


def assert_bits(got, want, what):
    """index equal, features equal as bit patterns (so that -0.0 and 0.0 differ and a NaN equals itself)"""
    (gf, gi), (wf, wi) = got, want
    assert gf.shape == wf.shape and gi.shape == wi.shape, what
    bad = np.argwhere(gi != wi)
    assert not len(bad), f'{what}: index differs at {bad[:8].tolist()}: kernel {gi[tuple(bad[0])]}, model {wi[tuple(bad[0])]}'
    bad = np.argwhere(gf.view(np.int32) != wf.view(np.int32))
    assert not len(bad), f'{what}: features differ at {bad[:8].tolist()}: kernel {gf[tuple(bad[0])]!r}, model {wf[tuple(bad[0])]!r}'


def test_the_definition_cases_through_the_entry_point():
    """B = 2, A = 3, E = 5, K = 4: an absent observer, an absent neighbour, the bit-equal tie, a neighbour at exactly r2 and one a float32 step
    beyond, one coincident with the observer, a NaN pose, K larger than the candidates (neighbors_model.definition_cases)"""
    c = nm.definition_cases()
    got = run(c, 3, 4, nm.DEFINITION_MAX_DISTANCE)
    assert got[1].tolist() == nm.DEFINITION_INDEX
    assert_bits(got, nm.neighbors(c['boxes'], c['sc'], c['speed'], c['present'], 3, 4, nm.DEFINITION_MAX_DISTANCE), 'definition cases')
    # every output is written in full: the same call into tensors that held something else
    from torchdrivesim_amd import _native as nat
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    features = torch.full((2, 3, 4, 8), float('nan'), device=DEV)
    index = torch.full((2, 3, 4), 99, dtype=torch.int32, device=DEV)
    nat.call('tds_neighbors_f32', torch.device(DEV), t['boxes'], t['sc'], t['speed'], t['present'].view(torch.uint8), None, features, index, 2, 3, 5, 4,
             nm.DEFINITION_MAX_DISTANCE)
    assert_bits((features.cpu().numpy(), index.cpu().numpy()), got, 'into used tensors')


@pytest.mark.parametrize('E', [6, 64, 65, 130])
def test_wave_and_stride_boundaries(E):
    """one lane per entity up to 64, the strided rounds above; K = 1, 8 and 32 (more slots than entities at E = 6); random float32 poses in a
    120 m square with duplicated positions; a radius and none"""
    B, A = 2, 5
    s = nm.random_scenes(100 + E, B, A, E)
    filled = 0
    for K in (1, 8, 32):
        for max_distance in (30.0, float('inf')):
            want = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], A, K, max_distance)
            assert_bits(run(s, A, K, max_distance), want, f'E={E} K={K} max_distance={max_distance}')
            filled += int((want[1] >= 0).sum())
    assert filled > 0


@pytest.mark.parametrize('A', [16, 17, 33])
def test_slices_of_observers_and_the_later_turns_of_a_wave(A):
    """a workgroup takes 16 observers, four per wave: one full slice, a second slice with one observer, a third; B = 2, K = 4, 40 entities (by
    rank) and 70 (in rounds), a fifth of the entities absent, observers among them"""
    for E in (40, 70):
        s = nm.random_scenes(3001 + 100 * A + E, 2, A, E, absent=0.2)
        want = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], A, 4, 50.0)
        assert not s['present'][:, :A].all() and (want[1][:, 16 * ((A - 1) // 16):A] >= 0).any()       # absent observers; the last slice sees somebody
        assert_bits(run(s, A, 4, 50.0), want, f'A={A} E={E}')


def test_the_entity_limit():
    """E = 1024, K = 32 equals the model; E = 1025 is refused with TDS_ELIMIT"""
    from torchdrivesim_amd import _native as nat
    s = nm.random_scenes(7, 1, 2, 1024, duplicates=0.02)
    s['present'][:, :2] = True
    want = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], 2, 32, 50.0)
    assert (want[1] >= 0).all()
    assert_bits(run(s, 2, 32, 50.0), want, 'E=1024')
    with pytest.raises(nat.TdsError, match='LDS') as err:
        run(nm.random_scenes(8, 1, 2, 1025), 2, 32, 50.0)
    assert err.value.code == nat.E_LIMIT


def test_the_visible_mask():
    B, A, E, K = 3, 6, 40, 8
    s = nm.random_scenes(21, B, A, E, side=60.0)
    visible = np.random.default_rng(22).random((B, A, E)) < 0.6
    want = nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], A, K, 40.0, visible=visible)
    assert_bits(run(s, A, K, 40.0, visible=visible), want, 'random mask (bool)')
    assert_bits(run(s, A, K, 40.0, visible=visible.astype(np.uint8) * 3), want, 'random mask (uint8)')
    plain = run(s, A, K, 40.0)
    assert_bits(run(s, A, K, 40.0, visible=np.ones((B, A, E), bool)), plain, 'all ones')
    assert (plain[1] != want[1]).any()
    # above 64 entities too
    s = nm.random_scenes(23, 2, 3, 100)
    visible = np.random.default_rng(24).random((2, 3, 100)) < 0.5
    assert_bits(run(s, 3, 16, 50.0, visible=visible), nm.neighbors(s['boxes'], s['sc'], s['speed'], s['present'], 3, 16, 50.0, visible=visible), 'E=100 mask')


@pytest.fixture(scope='module')
def town01():
    """what test_gpu_range_scan.make_sim takes, with Town01 alone"""
    import bench
    from torchdrivesim_amd import lanelet2
    from torchdrivesim_amd.mesh import BirdviewMesh
    lanes = lanelet2.load_lanelet_map(os.path.join(GOLDEN, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    v, f, vc, c = bench.load_town01()
    mesh = BirdviewMesh(verts=torch.from_numpy(v)[None], faces=torch.from_numpy(f.astype(np.int64))[None], categories=c, colors={}, zs={},
                        vert_category=torch.from_numpy(vc.astype(np.int64))[None])
    return [lanes], [mesh], [(v, f.astype(np.int64))]


def model_inputs(sim):
    """exactly what compute_neighbors hands to the kernel, as numpy arrays"""
    st = sim.get_all_agent_state()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1)
    return (boxes.cpu().numpy(), sim._heading_sc().cpu().numpy(), st[..., 3].contiguous().cpu().numpy(), sim.get_all_agent_present_mask().cpu().numpy())


def as_numpy(nb):
    return nb.features.cpu().numpy(), nb.index.cpu().numpy()


def absent_npc(states, present):
    present[1, 9] = False


@pytest.fixture(scope='module')
def sim(town01):
    """Town01, 3 scenes x (8 agents + 4 NPCs) placed by heuristic_initialize_batch, one NPC absent"""
    return make_sim(town01, [0, 0, 0], 8, seed=17, npc=4, edit=absent_npc)


def test_through_the_simulator(sim):
    from torchdrivesim_amd.simulator import Neighbors
    from torchdrivesim_amd.utils import relative
    A, K = 8, 6
    nb = sim.compute_neighbors(k=K, max_distance=80.0)
    assert isinstance(nb, Neighbors) and nb.features.shape == (3, A, K, 8) and nb.index.shape == (3, A, K) and not nb.features.requires_grad
    boxes, sc, speed, present = model_inputs(sim)
    assert_bits(as_numpy(nb), nm.neighbors(boxes, sc, speed, present, A, K, 80.0), 'compute_neighbors')
    assert bool(nb.mask.any()) and bool((nb.index != 9)[1].all()) and torch.equal(nb.mask, nb.index >= 0)
    assert_bits(as_numpy(sim.compute_neighbors()), nm.neighbors(boxes, sc, speed, present, A, 8, 50.0), 'the defaults')
    # the dense form of the reference, gathered at index
    dense = sim.get_all_agents_relative(exclude_self=False)                              # B x A x E x 6: x, y, psi, length, width, present
    E = dense.shape[2]
    idx = nb.index.clamp(min=0).long()
    got = torch.gather(dense, 2, idx.unsqueeze(-1).expand(-1, -1, -1, 6)).cpu().numpy().astype(np.float64)
    assert got.shape == (3, A, K, 6) and nb.take(sim.get_all_agent_size()).shape == (3, A, K, 2)
    mask = nb.mask.cpu().numpy()
    f = nb.features.cpu().numpy().astype(np.float64)
    # the yardstick: utils.relative in float32 against float64, on these poses, on the CPU
    st = sim.get_all_agent_state().cpu()
    rel = {}
    for dtype in (torch.float32, torch.float64):
        p = st.to(dtype)
        xy, psi = relative(origin_xy=p[:, :A, None, :2], origin_psi=p[:, :A, None, 2:3], target_xy=p[:, None, :, :2], target_psi=p[:, None, :, 2:3])
        rel[dtype] = torch.cat([xy, psi], -1).to(torch.float64).numpy()
    wrap = lambda d: (d + math.pi) % (2 * math.pi) - math.pi
    d = rel[torch.float32] - rel[torch.float64]
    yard = [float(np.abs(d[..., 0]).max()), float(np.abs(d[..., 1]).max()), float(np.abs(wrap(d[..., 2])).max())]
    diff = [float(np.abs(f[..., 0] - got[..., 0])[mask].max()), float(np.abs(f[..., 1] - got[..., 1])[mask].max()),
            float(np.abs(wrap(np.arctan2(f[..., 2], f[..., 3]) - got[..., 2]))[mask].max())]
    for name, dd, y in zip(('x', 'y', 'psi'), diff, yard):
        print(f'{name}: kernel against the dense form {dd:.3g}, utils.relative float32 against float64 {y:.3g} (bound {4 * y:.3g})')
    assert all(dd <= 4 * y for dd, y in zip(diff, yard)), (diff, yard)
    assert np.array_equal(f[..., 6:][mask], got[..., 3:5][mask]) and (got[..., 5][mask] == 1).all()
    assert torch.equal(nb.take(sim.get_all_agent_size())[nb.mask], nb.features[..., 6:][nb.mask])


def test_occluded_perception_composes(sim):
    """get_noisy_present_mask() of the occlusion noise model is a `visible`: the neighbours are the model's with that mask"""
    from torchdrivesim_amd.observation_noise import StandardSensingObservationNoise
    noisy = sim.copy()
    noisy.observation_noise_model = StandardSensingObservationNoise()
    visible = noisy.get_noisy_present_mask()
    assert visible.shape == (3, 8, 12) and visible.dtype == torch.bool
    nb = noisy.compute_neighbors(k=8, max_distance=60.0, visible=visible)
    boxes, sc, speed, present = model_inputs(noisy)
    assert_bits(as_numpy(nb), nm.neighbors(boxes, sc, speed, present, 8, 8, 60.0, visible=visible.cpu().numpy()), 'occlusion mask')
    seen = torch.gather(visible, 2, nb.index.clamp(min=0).long())
    assert bool(seen[nb.mask].all())
    with pytest.raises(ValueError, match='visible must be'):
        noisy.compute_neighbors(visible=visible[:, :4])


def equal(a, b):
    return torch.equal(a.features.view(torch.int32), b.features.view(torch.int32)) and torch.equal(a.index, b.index)


def rows(nb, idx):
    from torchdrivesim_amd.simulator import Neighbors
    return Neighbors(nb.features[idx], nb.index[idx])


def test_batch_plumbing_reproduces_the_rows_bit_for_bit(sim):
    from torchdrivesim_amd.parallel import shard_simulator
    kw = dict(k=5, max_distance=70.0)
    whole = sim.compute_neighbors(**kw)
    assert equal(sim.compute_neighbors(**kw), whole) and equal(sim.copy().compute_neighbors(**kw), whole)
    idx = [2, 0]
    assert equal(sim.select_batch_elements(idx, in_place=False).compute_neighbors(**kw), rows(whole, idx))
    assert equal(sim[[1]].compute_neighbors(**kw), rows(whole, [1]))
    assert equal(sim.extend(2, in_place=False).compute_neighbors(**kw), rows(whole, [0, 0, 1, 1, 2, 2]))
    shards = [shard_simulator(sim, rank, 2).compute_neighbors(**kw) for rank in range(2)]
    assert torch.equal(torch.cat([s.features for s in shards]).view(torch.int32), whole.features.view(torch.int32))
    assert torch.equal(torch.cat([s.index for s in shards]), whole.index)


def test_no_exposed_agents_and_empty_batches():
    from torchdrivesim_amd import _ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    features, index = _ops.neighbors(z(2, 4, 5), z(2, 4, 2), z(2, 4), z(2, 4, dtype=torch.bool), 0, 3, 50.0)
    assert features.shape == (2, 0, 3, 8) and index.shape == (2, 0, 3)
    features, index = _ops.neighbors(z(0, 4, 5), z(0, 4, 2), z(0, 4), z(0, 4, dtype=torch.bool), 2, 3, 50.0)
    assert features.shape == (0, 2, 3, 8) and index.shape == (0, 2, 3)


def test_a_captured_step_and_neighbors_replays_the_eager_bits(town01):
    """step + compute_neighbors captured on one stream into a graph, warmed up eagerly first; three replays equal eager"""
    live = make_sim(town01, [0] * 4, 8, seed=61, npc=2)
    ref = make_sim(town01, [0] * 4, 8, seed=61, npc=2)
    B, A = 4, 8
    g0 = torch.Generator(device='cpu').manual_seed(3)
    actions = (torch.rand(3, B, A, 2, generator=g0) * 2 - 1).to(DEV)
    state = live.get_state().clone()
    action = actions[0].clone()

    def step():
        live.kinematic_model.set_state(state)
        live.step(action)
        return live.compute_neighbors(k=8, max_distance=50.0), live.get_state()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nb, new = step()
        state_next = new.clone()
    for i in range(3):
        ref.kinematic_model.set_state(state.clone())
        ref.step(actions[i])
        want = ref.compute_neighbors(k=8, max_distance=50.0)
        action.copy_(actions[i])
        g.replay()
        torch.cuda.synchronize()
        assert equal(nb, want) and torch.equal(new, ref.get_state())
        assert bool(nb.mask.any())
        state.copy_(state_next)
