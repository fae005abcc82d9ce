"""The time-to-collision kernel (csrc/ttc.hip) on the device against the float64 model of its definition (tests/ttc_model.py): ttc as BIT PATTERNS
and index exactly, no row excepted -- through the entry point on the definition cases and random scenes, at the wave and stride boundaries and
at the entity limit, with a `visible` mask, through Simulator.compute_time_to_collision and its batch plumbing, and captured into a graph."""
import os

import numpy as np
import pytest
import torch

import ttc_model as tm
from conftest import GOLDEN
from test_gpu_range_scan import make_sim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF = float('inf')


def run(s, A, K, horizon, margin=0.0, visible=None):
    """_ops.time_to_collision on the scenes of a model generator -> numpy ttc, index"""
    from torchdrivesim_amd import _ops
    t = {k: torch.from_numpy(v).to(DEV) for k, v in s.items()}
    vis = None if visible is None else torch.from_numpy(visible).to(DEV)
    ttc, index = _ops.time_to_collision(t['boxes'], t['sc'], t['speed'], t['present'], A, K, horizon, margin, visible=vis)
    assert ttc.dtype == torch.float32 and index.dtype == torch.int32 and not ttc.requires_grad and ttc.shape == index.shape
    return ttc.cpu().numpy(), index.cpu().numpy()


def model(s, A, K, horizon, margin=0.0, visible=None):
    return tm.time_to_collision(s['boxes'], s['sc'], s['speed'], s['present'], A, K, horizon, margin, visible=visible)


def assert_bits(got, want, what):
    """index equal, ttc equal as bit patterns (so that -0.0 and 0.0 differ and a NaN equals itself)"""
    (gt, gi), (wt, wi) = got, want
    assert gt.shape == wt.shape and gi.shape == wi.shape, what
    bad = np.argwhere(gi != wi)
    assert not len(bad), f'{what}: index differs at {bad[:8].tolist()}: kernel {gi[tuple(bad[0])]}, model {wi[tuple(bad[0])]}'
    bad = np.argwhere(gt.view(np.int32) != wt.view(np.int32))
    assert not len(bad), f'{what}: ttc differs at {bad[:8].tolist()}: kernel {gt[tuple(bad[0])]!r}, model {wt[tuple(bad[0])]!r}'


def test_the_definition_cases_through_the_entry_point():
    """B = 2, A = 3, E = 6, K = 4 within 3 s: head-on, the same lane behind, a crossing in a tie with it, contact at exactly the horizon and a
    float32 step beyond, an absent observer, an overlapping pair whose lo is -0.0, a NaN pose, an absent NPC, K larger than the candidates
    (ttc_model.definition_cases)"""
    c = tm.definition_cases()
    got = run(c, 3, 4, tm.DEFINITION_HORIZON)
    assert got[1].tolist() == tm.DEFINITION_INDEX and np.array_equal(got[0], np.array(tm.DEFINITION_TTC, np.float32))
    assert_bits(got, model(c, 3, 4, tm.DEFINITION_HORIZON), 'definition cases')
    assert_bits(run(c, 3, 4, INF, 0.75), model(c, 3, 4, INF, 0.75), 'definition cases, a margin and no horizon')
    # every output is written in full: the same call into tensors that held something else
    from torchdrivesim_amd import _native as nat
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    ttc = torch.full((2, 3, 4), float('nan'), device=DEV)
    index = torch.full((2, 3, 4), 99, dtype=torch.int32, device=DEV)
    nat.call('tds_time_to_collision_f32', torch.device(DEV), t['boxes'], t['sc'], t['speed'], t['present'].view(torch.uint8), None, ttc, index, 2, 3, 6, 4,
             tm.DEFINITION_HORIZON, 0.0)
    assert_bits((ttc.cpu().numpy(), index.cpu().numpy()), got, 'into used tensors')


@pytest.mark.parametrize('E', [6, 64, 65, 130])
def test_wave_and_stride_boundaries(E):
    """one lane per entity up to 64, the strided rounds above; K = 1, 4 and 32 (more slots than entities at E = 6); a horizon and none; a margin
    and none; random float32 poses with duplicated positions, absent entities and a NaN speed"""
    s, A = tm.scenes(f'E{E}')
    filled = 0
    for K in (1, 4, 32):
        for horizon in (3.0, INF):
            for margin in (0.0, 0.5):
                want = model(s, A, K, horizon, margin)
                assert_bits(run(s, A, K, horizon, margin), want, f'E={E} K={K} horizon={horizon} margin={margin}')
                filled += int((want[1] >= 0).sum())
    assert filled > 0


@pytest.mark.parametrize('A', [16, 17, 33])
def test_slices_of_observers_and_the_later_turns_of_a_wave(A):
    """a workgroup takes 16 observers, four per wave: one full slice, a second slice with one observer, a third; B = 2, K = 4, 40 entities (by
    rank) and 70 (in rounds), a fifth of the entities absent, observers among them"""
    for E in (40, 70):
        s = tm.random_scenes(4000 + 100 * A + E, 2, A, E, absent=0.2)
        want = model(s, A, 4, INF, 0.25)
        assert not s['present'][:, :A].all() and (want[1][:, 16 * ((A - 1) // 16):A] >= 0).any()       # absent observers; the last slice meets somebody
        assert_bits(run(s, A, 4, INF, 0.25), want, f'A={A} E={E}')


def test_the_entity_limit():
    """E = 1024, K = 32 equals the model; E = 1025 is refused with TDS_ELIMIT"""
    from torchdrivesim_amd import _native as nat
    s, A = tm.scenes('E1024')
    want = model(s, A, 32, INF)
    assert (want[1] >= 0).all()
    assert_bits(run(s, A, 32, INF), want, 'E=1024')
    assert_bits(run(s, A, 32, 3.0, 0.5), model(s, A, 32, 3.0, 0.5), 'E=1024 within 3 s')
    with pytest.raises(nat.TdsError, match='LDS') as err:
        run(tm.random_scenes(8, 1, 2, 1025), 2, 32, 5.0)
    assert err.value.code == nat.E_LIMIT


def test_the_visible_mask():
    s, A = tm.scenes('mask40')
    B, E, K = 3, 40, 8
    visible = np.random.default_rng(22).random((B, A, E)) < 0.6
    want = model(s, A, K, 4.0, visible=visible)
    assert_bits(run(s, A, K, 4.0, visible=visible), want, 'random mask (bool)')
    assert_bits(run(s, A, K, 4.0, visible=visible.astype(np.uint8) * 3), want, 'random mask (uint8)')
    plain = run(s, A, K, 4.0)
    assert_bits(run(s, A, K, 4.0, visible=np.ones((B, A, E), bool)), plain, 'all ones')
    assert (plain[1] != want[1]).any()
    # above 64 entities too
    s, A = tm.scenes('mask100')
    visible = np.random.default_rng(24).random((2, A, 100)) < 0.5
    assert_bits(run(s, A, 16, INF, 0.25, visible=visible), model(s, A, 16, INF, 0.25, visible=visible), 'E=100 mask')


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
    """exactly what compute_time_to_collision hands to the kernel, as numpy arrays"""
    st = sim.get_all_agent_state()
    boxes = torch.cat([st[..., :2], sim.get_all_agent_size(), st[..., 2:3]], -1)
    return dict(boxes=boxes.cpu().numpy(), sc=sim._heading_sc().cpu().numpy(), speed=st[..., 3].contiguous().cpu().numpy(),
                present=sim.get_all_agent_present_mask().cpu().numpy())


def as_numpy(t):
    return t.ttc.cpu().numpy(), t.index.cpu().numpy()


def moving(states, present):
    """everybody drives at 4 .. 15 m/s; agent 1 of scene 0 stands on agent 0; agent 2 of scene 0 crawls 30 m ahead of agent 3, on its course (some
    2.5 s away); one NPC is absent"""
    B, E = states.shape[:2]
    states[..., 3] = 4.0 + 11.0 * torch.arange(B * E, device=states.device).reshape(B, E) / (B * E)
    states[0, 1, :2] = states[0, 0, :2]
    psi = states[0, 3, 2]
    states[0, 2, :2] = states[0, 3, :2] + 30.0 * torch.stack([torch.cos(psi), torch.sin(psi)])
    states[0, 2, 2] = psi
    states[0, 2, 3], states[0, 3, 3] = 2.0, 12.0
    present[1, 9] = False


@pytest.fixture(scope='module')
def sim(town01):
    """Town01, 3 scenes x (8 agents + 4 NPCs) placed by heuristic_initialize_batch"""
    return make_sim(town01, [0, 0, 0], 8, seed=17, npc=4, edit=moving)


def test_through_the_simulator(sim):
    from torchdrivesim_amd.simulator import TimeToCollision
    A, K = 8, 6
    t = sim.compute_time_to_collision(k=K, horizon=INF, margin=0.25)
    assert isinstance(t, TimeToCollision) and t.ttc.shape == (3, A, K) and t.index.shape == (3, A, K) and not t.ttc.requires_grad
    s = model_inputs(sim)
    want = model(s, A, K, INF, 0.25)
    assert_bits(as_numpy(t), want, 'compute_time_to_collision')
    assert bool(t.mask.any()) and bool((t.index != 9)[1].all()) and torch.equal(t.mask, t.index >= 0) and torch.equal(t.min, t.ttc[..., 0])
    assert t.min[0, 0].item() == 0.0 and t.index[0, 0, 0].item() == 1 and t.index[0, 1, 0].item() == 0            # the pair that overlaps
    met = t.index[0, 3].tolist()
    assert 2 in met and 1.5 < t.ttc[0, 3, met.index(2)].item() < 3.0                                             # the one crawling ahead
    assert bool((t.ttc[~t.mask] == INF).all()) and bool(torch.isfinite(t.ttc[t.mask]).all())
    assert_bits(as_numpy(sim.compute_time_to_collision()), model(s, A, 1, 5.0), 'the defaults')
    assert t.take(sim.get_all_agent_size()).shape == (3, A, K, 2)
    visible = torch.rand(3, A, 12, generator=torch.Generator().manual_seed(5)) < 0.5
    assert_bits(as_numpy(sim.compute_time_to_collision(k=3, horizon=INF, visible=visible.to(DEV))), model(s, A, 3, INF, visible=visible.numpy()), 'visible')
    with pytest.raises(ValueError, match='visible must be'):
        sim.compute_time_to_collision(visible=visible[:, :4].to(DEV))


def equal(a, b):
    return torch.equal(a.ttc.view(torch.int32), b.ttc.view(torch.int32)) and torch.equal(a.index, b.index)


def rows(t, idx):
    from torchdrivesim_amd.simulator import TimeToCollision
    return TimeToCollision(t.ttc[idx], t.index[idx])


def test_batch_plumbing_reproduces_the_rows_bit_for_bit(sim):
    from torchdrivesim_amd.parallel import shard_simulator
    kw = dict(k=5, horizon=INF, margin=0.1)
    whole = sim.compute_time_to_collision(**kw)
    assert bool(whole.mask.any())
    assert equal(sim.compute_time_to_collision(**kw), whole) and equal(sim.copy().compute_time_to_collision(**kw), whole)
    idx = [2, 0]
    assert equal(sim.select_batch_elements(idx, in_place=False).compute_time_to_collision(**kw), rows(whole, idx))
    assert equal(sim[[1]].compute_time_to_collision(**kw), rows(whole, [1]))
    assert equal(sim.extend(2, in_place=False).compute_time_to_collision(**kw), rows(whole, [0, 0, 1, 1, 2, 2]))
    shards = [shard_simulator(sim, rank, 2).compute_time_to_collision(**kw) for rank in range(2)]
    assert torch.equal(torch.cat([s.ttc for s in shards]).view(torch.int32), whole.ttc.view(torch.int32))
    assert torch.equal(torch.cat([s.index for s in shards]), whole.index)


def test_no_exposed_agents_and_empty_batches(town01):
    from torchdrivesim_amd import _ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    ttc, index = _ops.time_to_collision(z(2, 4, 5), z(2, 4, 2), z(2, 4), z(2, 4, dtype=torch.bool), 0, 3, 5.0)
    assert ttc.shape == (2, 0, 3) and index.shape == (2, 0, 3)
    ttc, index = _ops.time_to_collision(z(0, 4, 5), z(0, 4, 2), z(0, 4), z(0, 4, dtype=torch.bool), 2, 3, 5.0)
    assert ttc.shape == (0, 2, 3) and index.shape == (0, 2, 3)
    none = make_sim(town01, [0, 0], 0, seed=3, npc=3).compute_time_to_collision(k=2)                             # A = 0: NPCs alone observe nothing
    assert none.ttc.shape == (2, 0, 2) and none.index.shape == (2, 0, 2) and none.ttc.dtype == torch.float32 and none.index.dtype == torch.int32
    assert none.mask.shape == (2, 0, 2) and none.min.shape == (2, 0)


def test_a_captured_step_and_time_to_collision_replays_the_eager_bits(town01):
    """step + compute_time_to_collision captured on one stream into a graph, warmed up eagerly first; three replays, the state moving on between
    them, equal eager"""
    live = make_sim(town01, [0] * 4, 8, seed=61, npc=2, edit=moving)
    ref = make_sim(town01, [0] * 4, 8, seed=61, npc=2, edit=moving)
    B, A = 4, 8
    g0 = torch.Generator(device='cpu').manual_seed(3)
    actions = (torch.rand(3, B, A, 2, generator=g0) * 2 - 1).to(DEV)
    state = live.get_state().clone()
    action = actions[0].clone()
    kw = dict(k=4, horizon=INF, margin=0.5)

    def step():
        live.kinematic_model.set_state(state)
        live.step(action)
        return live.compute_time_to_collision(**kw), live.get_state()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t, new = step()
        state_next = new.clone()
    first = state.clone()
    for i in range(3):
        ref.kinematic_model.set_state(state.clone())
        ref.step(actions[i])
        want = ref.compute_time_to_collision(**kw)
        action.copy_(actions[i])
        g.replay()
        torch.cuda.synchronize()
        assert equal(t, want) and torch.equal(new, ref.get_state())
        assert bool(t.mask.any())
        state.copy_(state_next)
    assert not torch.equal(state, first)                                             # the state moved between the replays
