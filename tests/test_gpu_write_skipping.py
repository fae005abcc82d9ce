"""Renders into an owned image buffer leave alone the 128-byte lines that held background after the last render into the buffer and hold
background again (raster.hip: write_out_bits, the coverage record of include/tdship.h; _ops.write_skip_decision).  Every image here is compared
BIT FOR BIT with a render of the same scene into a fresh NaN-filled tensor with skipping switched off; poisoned buffers show which lines were
stored.  B = 2 scenes x 6 cameras on Town01.  The lines are tracked by the 4-wave kernel at three workgroups per CU: 256 x 256 with five keys (the
headline's shape) and with nine (five agent types: two strips of 128 columns), 192 x 192 with seven keys (three types; six word columns, 48 row
quads: a wave spans two word columns).  Every line is stored, and the library says so, at 256 x 256 with six keys (two types: the 8-wave kernel),
at 192 x 192 with five keys (four workgroups per CU) and at 200 x 200 (no multiple of 32)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, A, FOV = 2, 6, 35.0

LEVELS = dict(direction=2, vehicle=4, left_lane=12, joint_lane=13, right_lane=14, road=15)
COLORS = dict(road=(155, 155, 155), vehicle=(32, 74, 135), left_lane=(80, 127, 86), right_lane=(128, 0, 128), joint_lane=(255, 255, 255),
              direction=(100, 255, 255))
TYPES = dict(vehicle=(4, (32, 74, 135)), bicycle=(5, (255, 150, 40)), pedestrian=(6, (255, 64, 180)), ego=(3, (255, 0, 0)), ground_truth=(9, (196, 188, 165)))


def pack(rgb):
    return (rgb[0] << 16) | (rgb[1] << 8) | rgb[2]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def ops():
    from torchdrivesim_amd import _ops
    return _ops


@pytest.fixture(scope='module')
def world(ops, oracle):
    """the map, and per number of agent types (1, 2, 3, 5 -> 5, 6, 7, 9 keys) two scenes: S1 and S2 = S1 with every agent (and so every camera) moved on
    by three steps of 0.1 s at 8 m/s"""
    t = load_golden('town01_mesh.npz')
    verts, faces, cats = t['verts'], t['faces'], [str(c) for c in t['categories']]
    cat = np.asarray(t['vert_category'])[faces[:, 0]]
    levels = sorted({float(v) for v in LEVELS.values()} | {float(z) for z, _ in TYPES.values()}, reverse=True)
    smap = ops.StaticMap(np.asarray(verts, np.float32), np.asarray(faces, np.int32), np.array([LEVELS[cats[c]] for c in cat], np.float32),
                         np.array([pack(COLORS[cats[c]]) for c in cat], np.uint32), levels, device=DEV)
    road = verts[np.asarray(t['vert_category']) == cats.index('road')]
    out = dict(smap=smap)
    for n_types in (1, 2, 3, 5):
        gen = np.random.default_rng(40 + n_types)
        names = list(TYPES)[:n_types]
        anchor = road[gen.integers(0, len(road), (B, 1))]
        s1 = np.concatenate([anchor + gen.uniform(-20, 20, (B, A, 2)), gen.uniform(-np.pi, np.pi, (B, A, 1)), np.full((B, A, 1), 8.0)], -1).astype(np.float32)
        s2 = s1.copy()
        s2[..., 0] += 3 * 0.1 * 8.0 * np.cos(s1[..., 2])
        s2[..., 1] += 3 * 0.1 * 8.0 * np.sin(s1[..., 2])
        far = s1.copy()
        far[..., :2] = 1.0e6
        size = np.concatenate([gen.uniform(3.0, 6.0, (B, A, 1)), gen.uniform(1.5, 2.5, (B, A, 1))], -1).astype(np.float32)
        kind = gen.integers(0, n_types, (B, A))
        kind[:, :n_types] = np.arange(n_types)
        body = np.array([(smap.rank_of(TYPES[n][0]) << 24) | pack(TYPES[n][1]) for n in names], np.int64)
        dkey = (smap.rank_of(LEVELS['direction']) << 24) | pack(COLORS['direction'])
        keys = torch.from_numpy(np.stack([body[kind], np.full_like(kind, dkey)], -1)).to(torch.int32).to(DEV)
        out[n_types] = dict(S1=dev(s1), S2=dev(s2), FAR=dev(far), tmpl=dev(oracle.actor_template(size)), keys=keys,
                            mask=torch.ones(B, A, A, dtype=torch.bool, device=DEV), key_table=[int(k) for k in body] + [int(dkey)])
    return out


_fresh = {}


def render(ops, world, n_types, state, res, out, rows=slice(None), agents_of=None):
    """the scene `state` (its cameras: the agents themselves) into `out`; rows: the scenes of the batch that are rendered; agents_of: the agents
    drawn, where they are not `state`'s (cameras far away that see nothing)"""
    w = world[n_types]
    ag = (state if agents_of is None else agents_of)[rows].contiguous()
    st = state[rows].contiguous()
    return ops.raster_scene(world['smap'], ag, ops.heading_sc(ag[..., 2]), w['tmpl'][rows].contiguous(), w['keys'][rows].contiguous(), w['mask'][rows].contiguous(),
                            st[..., :2].contiguous(), ops.heading_sc(st[..., 2]), FOV, res, out=out, key_table=w['key_table'])


def fresh(ops, world, n_types, name, res, rows=slice(None)):
    """the reference of every comparison: the same scene into a NaN-filled torch tensor, skipping off; computed once per case"""
    key = (n_types, name, res, rows.start, rows.stop)
    if key not in _fresh:
        n = len(range(B)[rows])
        buf = torch.full((n, A, 3, res, res), float('nan'), device=DEV)
        ops.use_write_skipping = False
        try:
            w = world[n_types]
            if name == 'FAR':
                render(ops, world, n_types, w['FAR'], res, buf, rows, agents_of=w['S1'])
            else:
                render(ops, world, n_types, w[name], res, buf, rows)
        finally:
            ops.use_write_skipping = True
        assert not torch.isnan(buf).any()
        _fresh[key] = buf
    return _fresh[key]


def record_of(ops, buf):
    """the buffer's coverage record, None unless the last render into it maintained one"""
    rec = ops._owned_buffers[buf.data_ptr()]['record']
    return rec if rec is not None and rec['valid'] else None


def tracks(n_types, res):
    """does the launch of this case keep a coverage record?  A side that is a multiple of 32, and the 4-wave kernel at three workgroups per CU
    (tests/test_raster_plan.py pins which shapes it serves)"""
    return (n_types, res) in ((1, 256), (5, 256), (3, 192))


CASES = [(1, 256), (3, 192), (5, 256), (1, 192), (1, 200), (2, 256)]


@pytest.mark.parametrize('n_types,res', CASES)
def test_a_second_scene_over_the_first(ops, world, n_types, res):
    w = world[n_types]
    buf = ops.owned_image((B, A, 3, res, res), torch.float32, DEV)
    assert render(ops, world, n_types, w['S1'], res, buf) is buf
    assert torch.equal(buf, fresh(ops, world, n_types, 'S1', res))
    render(ops, world, n_types, w['S2'], res, buf)
    assert torch.equal(buf, fresh(ops, world, n_types, 'S2', res))
    assert not torch.equal(fresh(ops, world, n_types, 'S1', res), fresh(ops, world, n_types, 'S2', res))
    assert (record_of(ops, buf) is not None) == tracks(n_types, res)


@pytest.mark.parametrize('n_types,res', [(1, 256), (3, 192)])
def test_covered_to_background_and_back(ops, world, n_types, res):
    w = world[n_types]
    buf = ops.owned_image((B, A, 3, res, res), torch.float32, DEV)
    render(ops, world, n_types, w['S1'], res, buf)
    assert torch.equal(buf, fresh(ops, world, n_types, 'S1', res))
    render(ops, world, n_types, w['FAR'], res, buf, agents_of=w['S1'])
    assert torch.equal(buf, fresh(ops, world, n_types, 'FAR', res)) and not buf.any()
    render(ops, world, n_types, w['S1'], res, buf)
    assert torch.equal(buf, fresh(ops, world, n_types, 'S1', res))


def test_a_fill_between_two_renders_is_seen(ops, world):
    w = world[1]
    buf = ops.owned_image((B, A, 3, 256, 256), torch.float32, DEV)
    render(ops, world, 1, w['S1'], 256, buf)
    buf.fill_(float('nan'))
    render(ops, world, 1, w['S2'], 256, buf)
    assert not torch.isnan(buf).any() and torch.equal(buf, fresh(ops, world, 1, 'S2', 256))


def poison(buf):
    buf.data.fill_(7.0)            # through .data: the version counter of `buf` does not move


def test_other_shapes_views_and_capture_store_every_line(ops, world):
    w = world[1]
    buf = ops.owned_image((B, A, 3, 256, 256), torch.float32, DEV)
    whole = lambda: (poison(buf), render(ops, world, 1, w['S1'], 256, buf), torch.equal(buf, fresh(ops, world, 1, 'S1', 256)))[2]
    render(ops, world, 1, w['S1'], 256, buf)
    assert record_of(ops, buf) is not None
    # the same storage through another resolution
    small = buf.view(-1)[:B * A * 3 * 192 * 192].view(B, A, 3, 192, 192)
    poison(buf)
    render(ops, world, 1, w['S1'], 192, small)
    assert torch.equal(small, fresh(ops, world, 1, 'S1', 192)) and record_of(ops, buf) is None
    assert whole()                                                    # ... after which the whole buffer is stored again
    # half the batch, at the buffer's address and behind it
    for rows in (slice(0, 1), slice(1, 2)):
        assert record_of(ops, buf) is not None
        poison(buf)
        render(ops, world, 1, w['S1'], 256, buf[rows], rows)
        assert torch.equal(buf[rows], fresh(ops, world, 1, 'S1', 256, rows)) and record_of(ops, buf) is None
        assert whole()
    # under stream capture: the graph stores every line at every replay and holds no record
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        render(ops, world, 1, w['S1'], 256, buf)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        render(ops, world, 1, w['S1'], 256, buf)
    assert record_of(ops, buf) is None
    for _ in range(2):
        poison(buf)
        g.replay()
        assert torch.equal(buf, fresh(ops, world, 1, 'S1', 256))
    assert whole() and record_of(ops, buf) is not None
    del g


@pytest.mark.parametrize('n_types,res', [(1, 256), (3, 192), (5, 256), (1, 192), (1, 200), (2, 256)])
def test_exactly_the_background_lines_are_left_alone(ops, world, n_types, res):
    """S1 twice, the buffer poisoned in between behind the version counter's back: the 7s that survive lie in lines whose 32 pixels are background in
    S1 (safety), and every such line survives in all three channels (what the launch saves).  Where the lines are not tracked nothing survives."""
    w = world[n_types]
    ref = fresh(ops, world, n_types, 'S1', res)
    buf = ops.owned_image((B, A, 3, res, res), torch.float32, DEV)
    render(ops, world, n_types, w['S1'], res, buf)
    poison(buf)
    render(ops, world, n_types, w['S1'], res, buf)
    if not tracks(n_types, res):
        assert record_of(ops, buf) is None and torch.equal(buf, ref)
        return
    # a line: 32 pixels along the last axis, one per channel; background where all three channels are zero over all of them
    lines = (ref != 0).view(B, A, 3, res, res // 32, 32).any(-1).any(2, keepdim=True).expand(B, A, 3, res, res // 32)
    stored = lines[..., None].expand(B, A, 3, res, res // 32, 32).reshape(B, A, 3, res, res)
    survived = buf == 7.0
    assert not (survived & stored).any()
    assert torch.equal(buf[stored], ref[stored])
    assert survived[~stored].all()
    share = 1.0 - lines.float().mean().item()
    print(f'{n_types} agent types, {res} x {res}: {share:.3f} of the lines left alone')
    assert share > 0.0
