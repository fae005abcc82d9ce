"""The stream-out of the bit-plane kernels (raster.hip: write_out_bits) against the ORACLE, byte for byte.  tests/test_gpu_write_skipping.py compares two
renders of the same kernel, which a stream-out that is wrong in both passes; here every image is oracle.render_scenes' image of the same scene.
B = 2 scenes x 6 cameras on Town01, the smallest shapes that reach each form of the function:

    40 x 40, 5 keys     a side that is a multiple of 4 but not of 32: a partial word column, the bounds-checked emit
    64 x 64, 5 keys     the split form's raster_list_bits_kernel
    192 x 192, 5 keys   four workgroups per CU
    192 x 192, 7 keys   persistent, tracked, a wave spans two word columns
    256 x 256, 5 keys   the headline's instantiation
    256 x 256, 6 keys   the 8-wave kernel
    256 x 256, 9 keys   two strips, four index bits
    256 x 256, 5 keys, differentiable: the instantiation that also emits the index slices

Every shape is rendered three ways into one owned buffer: into the fresh buffer, again after the cameras moved (where the lines are tracked,
covered-then-background lines are rewritten and background-twice lines are left alone), and once more with skipping off."""
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
#: (agent types, resolution): 1, 2, 3, 5 types are 5, 6, 7, 9 distinct keys
SHAPES = [(1, 40), (1, 64), (1, 192), (3, 192), (1, 256), (2, 256), (5, 256)]


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
    """the map (the product's and the oracle's arrays of it), and per number of agent types two scenes: S1 and S2 = S1 with every agent (and so every
    camera) moved on by three steps of 0.1 s at 8 m/s"""
    t = load_golden('town01_mesh.npz')
    verts, faces, cats = t['verts'], t['faces'], [str(c) for c in t['categories']]
    cat = np.asarray(t['vert_category'])[faces[:, 0]]
    levels = sorted({float(v) for v in LEVELS.values()} | {float(z) for z, _ in TYPES.values()}, reverse=True)
    smap = ops.StaticMap(np.asarray(verts, np.float32), np.asarray(faces, np.int32), np.array([LEVELS[cats[c]] for c in cat], np.float32),
                         np.array([pack(COLORS[cats[c]]) for c in cat], np.uint32), levels, device=DEV)
    static = oracle.static_mesh_arrays(verts, faces, t['vert_category'], cats, colors={**oracle.DEFAULT_COLORS, **COLORS},
                                       levels={**oracle.DEFAULT_LEVELS, **LEVELS})
    road = verts[np.asarray(t['vert_category']) == cats.index('road')]
    out = dict(smap=smap, static=static)
    for n_types in (1, 2, 3, 5):
        gen = np.random.default_rng(40 + n_types)
        names = list(TYPES)[:n_types]
        anchor = road[gen.integers(0, len(road), (B, 1))]
        s1 = np.concatenate([anchor + gen.uniform(-20, 20, (B, A, 2)), gen.uniform(-np.pi, np.pi, (B, A, 1)), np.full((B, A, 1), 8.0)], -1).astype(np.float32)
        s2 = s1.copy()
        s2[..., 0] += 3 * 0.1 * 8.0 * np.cos(s1[..., 2])
        s2[..., 1] += 3 * 0.1 * 8.0 * np.sin(s1[..., 2])
        size = np.concatenate([gen.uniform(3.0, 6.0, (B, A, 1)), gen.uniform(1.5, 2.5, (B, A, 1))], -1).astype(np.float32)
        kind = gen.integers(0, n_types, (B, A))
        kind[:, :n_types] = np.arange(n_types)
        body = np.array([(smap.rank_of(TYPES[n][0]) << 24) | pack(TYPES[n][1]) for n in names], np.int64)
        dkey = (smap.rank_of(LEVELS['direction']) << 24) | pack(COLORS['direction'])
        keys = torch.from_numpy(np.stack([body[kind], np.full_like(kind, dkey)], -1)).to(torch.int32).to(DEV)
        lev = np.stack([np.array([TYPES[n][0] for n in names], np.float32)[kind], np.full(kind.shape, LEVELS['direction'], np.float32)], -1)
        col = np.stack([np.array([TYPES[n][1] for n in names], np.float32)[kind],
                        np.broadcast_to(np.array(COLORS['direction'], np.float32), kind.shape + (3,))], -2) / np.float32(255.0)
        out[n_types] = dict(S1=dev(s1), S2=dev(s2), size=size, lev=lev, col=col.astype(np.float32), tmpl=dev(oracle.actor_template(size)), keys=keys,
                            mask=torch.ones(B, A, A, dtype=torch.bool, device=DEV), key_table=[int(k) for k in body] + [int(dkey)])
    return out


_expected = {}


def expected(ops, oracle, world, n_types, name, res):
    """the oracle's image of scene `name` (headings as the product's sine / cosine pairs, as everywhere in the suite); computed once per case"""
    key = (n_types, name, res)
    if key not in _expected:
        w = world[n_types]
        state = w[name].cpu().numpy()
        sc = ops.heading_sc(w[name][..., 2]).cpu().numpy()
        ref = oracle.render_scenes(state, w['size'], np.ones((B, A, A), bool), state[..., :2].copy(), sc, *world['static'], FOV, res, agent_sc=sc,
                                   actor_levels=w['lev'], actor_colors=w['col'])
        assert ref.dtype == np.float32 and (ref > 0).any()
        ref.setflags(write=False)
        _expected[key] = ref
    return _expected[key]


def same_bytes(img, ref):
    got = img.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    return np.array_equal(got.view(np.uint8), ref.view(np.uint8))


def render(ops, world, n_types, name, res, **kw):
    w = world[n_types]
    st = w[name]
    sc = ops.heading_sc(st[..., 2])
    return ops.raster_scene(world['smap'], st, sc, w['tmpl'], w['keys'], w['mask'], st[..., :2].contiguous(), sc, FOV, res, key_table=w['key_table'], **kw)


@pytest.mark.parametrize('n_types,res', SHAPES)
def test_float32_images_are_the_oracles(ops, oracle, world, n_types, res):
    s1, s2 = expected(ops, oracle, world, n_types, 'S1', res), expected(ops, oracle, world, n_types, 'S2', res)
    assert not np.array_equal(s1, s2)
    buf = ops.owned_image((B, A, 3, res, res), torch.float32, DEV)
    buf.fill_(float('nan'))
    assert render(ops, world, n_types, 'S1', res, out=buf) is buf
    assert same_bytes(buf, s1), 'into a fresh buffer'
    render(ops, world, n_types, 'S2', res, out=buf)
    assert same_bytes(buf, s2), 'after the cameras moved'
    render(ops, world, n_types, 'S1', res, out=buf, write_skipping=False)
    assert same_bytes(buf, s1), 'skipping off'
    # and without a caller's buffer
    assert same_bytes(render(ops, world, n_types, 'S2', res), s2)


def test_uint8_is_unchanged(ops, oracle, world):
    ref = expected(ops, oracle, world, 1, 'S1', 256)
    img = render(ops, world, 1, 'S1', 256, out_dtype=torch.uint8)
    assert img.dtype == torch.uint8
    assert np.array_equal(img.cpu().numpy().astype(np.float32), ref)


def test_differentiable_forward_and_its_index_slices(ops, oracle, world):
    """the instantiation that also stores the resolved key index: the image is the oracle's, and the index slices (include/tdship.h: per camera, word
    column and row quad 64 bytes = four slices of four rows, bit p of slice b = bit b of the index of column 32 xw + p) name the image's colours"""
    res = 256
    ref = expected(ops, oracle, world, 1, 'S1', res)
    img, slices, keys = render(ops, world, 1, 'S1', res, index_slices=True)
    assert slices is not None and same_bytes(img, ref)
    wpw, quads = res // 32, res // 4
    s = slices.cpu().numpy().view(np.uint32)[:B * A * wpw * quads * 16].reshape(B * A, wpw, quads, 4, 4)                  # [camera, xw, row quad, slice, row]
    bits = (s[..., None] >> np.arange(32, dtype=np.uint32)) & 1                                 # [..., column within the word]
    idx = (bits << np.arange(4, dtype=np.uint32)[None, None, None, :, None, None]).sum(3)       # [camera, xw, row quad, row, column]
    idx = idx.transpose(0, 1, 4, 2, 3).reshape(B * A, res, res)                                 # [camera, x, y]
    table = np.array([0] + [int(k) & 0xffffffff for k in keys], np.uint32)
    assert 0 < idx.max() < len(table)
    rgb = table[idx]
    named = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], 1).astype(np.float32).reshape(B, A, 3, res, res)
    assert np.array_equal(named, ref)
