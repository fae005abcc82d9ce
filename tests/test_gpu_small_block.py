"""The block that paints small faces on the lane that scanned them (raster.hip: process_small_bits<ROWS>) takes the slopes of its short edges
without a division (tds_short_slope.h: edge_dx_short) and paints the rows between the vertices in one form.  The slope can only go wrong on
shapes no real map has -- FLAT WIDE faces, two to seven rows high and up to the image's width across -- so this file renders a map of those:
one scene x 8 cameras at 256 x 256 (the smallest side at which the persistent five-key instantiation runs) as float32, uint8 and index slices.
Every image equals the oracle's byte for byte and equals the render with the path off (small_faces=False), in the testing build and in the
product; the testing build's counter shows that the faces took the path.  One case at 128 x 128 goes through the split form, whose list
rasteriser holds the block's four-row instantiation: the same shapes at that resolution, against the oracle and against the launch without
the short path (TDS_RASTER_DBG_NO_SHORT_PATH)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_map, oracle_static
from test_gpu_small_faces import CATS, FOV, pixel_to_world, project, reference, render, scene, small_stats

pytestmark = pytest.mark.gpu
RES, ROWS = 256, 7
LIST_RES, LIST_ROWS = 128, 4             # the split form's resolution and the rows its list rasteriser paints on the lane
MIN_WIDTH = 8


@pytest.fixture(scope='module')
def ops():
    from torchdrivesim_amd import _ops
    return _ops


def flat_wide_map(res, rows):
    """faces designed in the pixels of camera 0 (at the origin, looking along x): every height of 2 .. `rows` rows, the middle vertex in every
    row from the top (ym == yt) to the bottom (ym == yb), widths stepping from 8 pixels to res - 1, the long edge T -> B running left to right
    and right to left, the middle vertex between, left of and right of it, the three vertices in every order; all vertices inside the image,
    at pixel centres, so that the truncation of the projection cannot move them.  About two thousand faces over one 35 m view."""
    verts, faces, cat = [], [], []
    orders = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    n = 0
    for h in range(1, rows):
        for m in range(h + 1):
            widths = list(range(MIN_WIDTH + (3 * h + m) % 9, res, 19)) + [res - 1 - (h + m) % 3]
            for wid in widths:
                for kind in range(6):
                    fwd, pos = kind & 1, kind >> 1
                    x0, y0 = (n * 53) % (res - wid), (n * 29) % (res - h)
                    xT, xB = (x0, x0 + wid) if fwd else (x0 + wid, x0)
                    xM = x0 + wid // 3 if pos == 0 else (x0 if pos == 1 else x0 + wid)
                    tri = [(xT, y0), (xM, y0 + m), (xB, y0 + h)]
                    k = len(verts)
                    for i in orders[n % 6]:
                        verts.append(pixel_to_world((tri[i][0] + 0.5, tri[i][1] + 0.5), (0.0, 0.0), 0.0, FOV, res))
                    faces.append((k, k + 1, k + 2)); cat.append(n % 3)
                    n += 1
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int32)
    vcat = np.zeros(len(verts), np.int64)
    vcat[faces[:, 0]] = cat; vcat[faces[:, 1]] = cat; vcat[faces[:, 2]] = cat
    return verts, faces, vcat


def cameras(res):
    """camera 0 sees the faces as designed; the others turn them by half a turn, move them by fractions of a pixel and by whole pixels (some
    faces then cross the border and are not small), tilt them slightly (wide faces gain rows) and turn them upright (none is small)"""
    px = FOV / res
    psi = np.array([0.0, np.pi, 0.0, 0.0, np.pi / 2, 0.004, np.pi, 0.0], np.float32)
    xy = np.array([[0, 0], [0, 0], [0.3 * px, 0.4 * px], [20.25 * px, 0], [0, 0], [0, 0], [0.45 * px, -2.3 * px], [-7.5 * px, 3.25 * px]], np.float32)
    return xy[None], psi[None]


def pixel_boxes(verts, faces, cam_xy, psi, res):
    X, Y = project(verts, cam_xy, psi, res, FOV)
    return X[faces], Y[faces]


def count_small(verts, faces, cam_xy, psi, res, rows):
    """the faces the kernels' test calls small (all three vertices inside the image, at most `rows` rows), over all cameras"""
    n = 0
    for k in range(cam_xy.shape[1]):
        X, Y = pixel_boxes(verts, faces, cam_xy[0, k], psi[0, k], res)
        inside = ((X >= 0) & (X < res) & (Y >= 0) & (Y < res)).all(1)
        n += int((inside & (Y.max(1) - Y.min(1) <= rows - 1)).sum())
    return n


@pytest.mark.parametrize('res,rows', [(RES, ROWS), (LIST_RES, LIST_ROWS)])
def test_the_map_holds_the_cases_it_claims(res, rows):
    verts, faces, _ = flat_wide_map(res, rows)
    cam_xy, psi = cameras(res)
    X, Y = pixel_boxes(verts, faces, cam_xy[0, 0], psi[0, 0], res)
    assert ((X >= 0) & (X < res) & (Y >= 0) & (Y < res)).all()
    h, wid = Y.max(1) - Y.min(1), X.max(1) - X.min(1)
    assert 300 <= len(faces) <= 4000
    assert h.min() == 1 and h.max() == rows - 1 and wid.min() >= MIN_WIDTH and wid.max() == res - 1
    for want in range(1, rows):                                # every height, and in it the middle vertex in every row
        assert (h == want).sum() >= 5, want
        ym = np.sort(Y, 1)[:, 1] - Y.min(1)
        for m in range(want + 1):
            assert ((h == want) & (ym == m)).sum() >= 5, (want, m)
    lo = MIN_WIDTH
    while lo < res:                                            # every width octave, in every height
        for want in range(1, rows):
            assert ((wid >= lo) & (wid < 2 * lo) & (h == want)).sum() >= 5, (lo, want)
        lo *= 2
    # both directions of the long edge, and every one of the six vertex orders
    top, bot = np.argmin(Y * 65536 + X, 1), np.argmax(Y * 65536 + X, 1)
    xt, xb = X[np.arange(len(X)), top], X[np.arange(len(X)), bot]
    assert (xt < xb).sum() >= 100 and (xt > xb).sum() >= 100
    assert len(set(zip(top.tolist(), bot.tolist()))) == 6
    # the other cameras keep most of them small, and the upright one none
    X4, Y4 = pixel_boxes(verts, faces, cam_xy[0, 4], psi[0, 4], res)
    assert ((Y4.max(1) - Y4.min(1)) >= MIN_WIDTH).all()
    assert count_small(verts, faces, cam_xy, psi, res, rows) >= 4 * len(faces)


@pytest.mark.parametrize('mode', ['float32', 'uint8', 'slices'])
def test_flat_wide_faces_equal_the_oracle_on_and_off_the_path(ops, oracle, mode):
    from torchdrivesim_amd import _native as nat
    verts, faces, vcat = flat_wide_map(RES, ROWS)
    cam_xy, psi = cameras(RES)
    n_small = count_small(verts, faces, cam_xy, psi, RES, ROWS)
    state, size, mask = scene(oracle, 1, 8, np.random.default_rng(9))
    ref = reference(ops, oracle, oracle_static(oracle, verts, faces, vcat, CATS), state, size, mask, cam_xy, psi, RES)
    kw = dict(out_dtype=torch.uint8) if mode == 'uint8' else (dict(index_slices=True) if mode == 'slices' else {})
    image = lambda r: (r[0] if isinstance(r, tuple) else r).cpu().numpy()
    with nat.testing() as T:
        smap = make_map(ops, verts, faces, vcat, CATS)
        try:
            T.tds_raster_set_debug(int(nat.RasterDebug.STATS))
            small_stats(T)
            on = image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, **kw))
            torch.cuda.synchronize()
            s_on = small_stats(T)
            off = image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, small_faces=False, **kw))
            torch.cuda.synchronize()
            s_off = small_stats(T)
        finally:
            T.tds_raster_set_debug(0)
        del smap
    print(f'{mode}: faces painted on their lane {s_on[15]} of {s_on[1] + s_on[3]} accepted ({s_on[2] + s_on[4]} small; the CPU projection calls '
          f'{n_small} of the map\'s small); path off: {s_off[15]}')
    assert 2 * s_on[15] >= n_small and s_off[15] == 0
    assert s_on[1] == s_off[1] and s_on[2] == s_off[2] == n_small        # the kernel's test and the projection here agree on what is small
    assert np.array_equal(on, ref.astype(on.dtype)), int((on != ref).any((2, 3, 4)).sum())
    assert np.array_equal(off, on)
    # the product library, with the path and, through the module switch of _ops, without it
    smap = make_map(ops, verts, faces, vcat, CATS)
    assert np.array_equal(image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, **kw)), on)
    ops.use_small_faces = False
    try:
        assert np.array_equal(image(render(ops, oracle, smap, state, size, mask, cam_xy, psi, RES, **kw)), on)
    finally:
        ops.use_small_faces = True


def test_the_list_rasteriser_paints_them_in_four_rows(ops, oracle):
    """128 x 128 runs as the split form; its list rasteriser paints faces of up to four rows with the same block"""
    from test_raster_plan import SPLIT, plan
    from torchdrivesim_amd import _native as nat
    assert plan(LIST_RES, 5, n_img=8)['form'] == SPLIT
    verts, faces, vcat = flat_wide_map(LIST_RES, LIST_ROWS)
    cam_xy, psi = cameras(LIST_RES)
    assert count_small(verts, faces, cam_xy, psi, LIST_RES, LIST_ROWS) >= 4 * len(faces)
    state, size, mask = scene(oracle, 1, 8, np.random.default_rng(9))
    ref = reference(ops, oracle, oracle_static(oracle, verts, faces, vcat, CATS), state, size, mask, cam_xy, psi, LIST_RES)
    with nat.testing() as T:
        smap = make_map(ops, verts, faces, vcat, CATS)
        try:
            on = render(ops, oracle, smap, state, size, mask, cam_xy, psi, LIST_RES).cpu().numpy()
            T.tds_raster_set_debug(int(nat.RasterDebug.NO_SHORT_PATH))
            off = render(ops, oracle, smap, state, size, mask, cam_xy, psi, LIST_RES).cpu().numpy()
        finally:
            T.tds_raster_set_debug(0)
        del smap
    assert np.array_equal(on, ref), int((on != ref).any((2, 3, 4)).sum())
    assert np.array_equal(off, on)
    smap = make_map(ops, verts, faces, vcat, CATS)
    assert np.array_equal(render(ops, oracle, smap, state, size, mask, cam_xy, psi, LIST_RES).cpu().numpy(), on)
