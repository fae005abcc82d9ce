"""Which launches K3 (the scene rasteriser) makes for a call of a given shape: raster.hip's plan_raster_scene through the testing hook
tds_raster_plan, on the CPU.  Every form paints the same pixels, so the GPU parity tests cannot see a change of form; this table can.
The expected plans are the rules as they stand (including the ones a later change may want to revisit, such as eight waves ruling out the
split form for uint8 at 192 - 216 px with 8 - 10 keys)."""
import ctypes

import pytest

from torchdrivesim_amd import _native
from torchdrivesim_amd._native import OUT_F32, OUT_U8, RasterDebug as D

BITS, SPLIT, BINNED, FUSED, ELIMIT = range(5)


class Plan(ctypes.Structure):
    """tds_raster_plan_t (include/tdship.h, testing hooks)"""
    _fields_ = [(n, ctypes.c_int) for n in ('form', 'tw', 'strips', 'twp', 'nwv', 'nb', 'minwg', 'emit', 'four_per_cu', 'persist', 'tws', 'lw')] + \
               [(n, ctypes.c_int64) for n in ('lds', 'lds_s', 'grid', 'caps', 'off_counts', 'off_lists', 'off_lists3')]


def workspace(n_img, res, out_mode, n_keys):
    """the workspace _ops allocates for the call (tds_raster_scene_workspace_bytes_for of the product)"""
    n = ctypes.c_int64()
    _native.check(_native.lib().tds_raster_scene_workspace_bytes_for(n_img, res, out_mode, n_keys, ctypes.byref(n)), 'workspace_bytes_for')
    return n.value


def plan(res, keys, out_mode=OUT_F32, n_img=65536, listed=True, actors=True, extra=False, slices=False, ws=None, cus=256,
         force_tw=0, bits_waves=4, list_waves=0, list_lds_kb=40, debug=0):
    """keys: distinct keys of the scene (-1: more than 15); ws: workspace bytes (None: what the product recommends, 0: none)"""
    if ws is None:
        ws = workspace(n_img, res, out_mode, keys)
    p = Plan()
    _native.check(_native.testing_lib().tds_raster_plan(n_img, res, out_mode, keys, int(listed), int(actors), int(extra), int(slices), ws, cus,
                                                        force_tw, bits_waves, list_waves, list_lds_kb, int(debug), ctypes.byref(p)), 'tds_raster_plan')
    return {name: getattr(p, name) for name, _ in Plan._fields_}


# (name, call, expected): B x A = 65 536 cameras, 256 CUs, the recommended workspace and the default knobs unless the call says otherwise.
# The bench headline is the first row: float32 256 x 256, Town01's keys -- the persistent 4-wave bit-plane kernel with MINWG = 3,
# raster_scene_bits_kernel<4, 3, float, SceneArgs, false, 3> of profiles/r0*_bench_kernel_stats.csv.
CASES = [
    ('headline f32 256 4 keys', dict(res=256, keys=4), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('headline f32 256 5 keys', dict(res=256, keys=5), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('headline 224 CUs (reserved stream)', dict(res=256, keys=5, cus=224), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=672)),
    ('f32 256 1 keys', dict(res=256, keys=1), dict(form=BITS, twp=256, strips=1, nwv=4, nb=2, minwg=4, emit=0, persist=0, grid=65536)),
    ('f32 256 2 keys', dict(res=256, keys=2), dict(form=BITS, twp=256, strips=1, nwv=4, nb=2, minwg=4, emit=0, persist=0, grid=65536)),
    ('f32 256 3 keys', dict(res=256, keys=3), dict(form=BITS, twp=256, strips=1, nwv=4, nb=2, minwg=4, emit=0, persist=0, grid=65536)),
    ('f32 256 6 keys', dict(res=256, keys=6), dict(form=BITS, twp=256, strips=1, nwv=8, nb=3, minwg=0, emit=0, persist=0, grid=65536)),
    ('f32 256 7 keys', dict(res=256, keys=7), dict(form=BITS, twp=256, strips=1, nwv=8, nb=3, minwg=0, emit=0, persist=0, grid=65536)),
    ('f32 256 8 keys', dict(res=256, keys=8), dict(form=BITS, twp=128, strips=2, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=768)),
    ('f32 256 9 keys', dict(res=256, keys=9), dict(form=BITS, twp=128, strips=2, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=768)),
    ('f32 256 10 keys', dict(res=256, keys=10), dict(form=BITS, twp=96, strips=3, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=768)),
    ('f32 256 15 keys', dict(res=256, keys=15), dict(form=BITS, twp=128, strips=2, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=512)),
    ('u8 256 6 keys', dict(res=256, keys=6, out_mode=OUT_U8), dict(form=BITS, twp=256, strips=1, nwv=8, nb=3, minwg=0, emit=0, persist=0, grid=65536)),
    ('u8 256 7 keys', dict(res=256, keys=7, out_mode=OUT_U8), dict(form=BITS, twp=256, strips=1, nwv=8, nb=3, minwg=0, emit=0, persist=0, grid=65536)),
    ('u8 256 8 keys', dict(res=256, keys=8, out_mode=OUT_U8), dict(form=BITS, twp=128, strips=2, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=768)),
    ('16+ keys, workspace: binned', dict(res=256, keys=-1), dict(form=BINNED, tw=64, strips=4, caps=512)),
    ('16+ keys, no workspace: fused', dict(res=256, keys=-1, ws=0), dict(form=FUSED, tw=64, strips=4, grid=262144)),
    ('actor keys not listed: fused', dict(res=256, keys=5, listed=False, ws=0), dict(form=FUSED, tw=64, strips=4, grid=262144)),
    ('actor keys not listed, workspace sized for bit planes', dict(res=256, keys=5, listed=False), dict(form=FUSED, tw=64, strips=4, grid=262144)),
    ('static map only needs no listed keys', dict(res=256, keys=5, listed=False, actors=False), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('per-camera triangles need listed keys', dict(res=256, keys=5, listed=False, actors=False, extra=True), dict(form=FUSED, tw=64, strips=4, grid=262144)),
    ('u8 64 5 keys', dict(res=64, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=64, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 64 5 keys', dict(res=64, keys=5, out_mode=OUT_F32), dict(form=SPLIT, tws=64, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('u8 108 5 keys', dict(res=108, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=128, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 108 5 keys', dict(res=108, keys=5, out_mode=OUT_F32), dict(form=SPLIT, tws=128, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('u8 112 5 keys', dict(res=112, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=128, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 112 5 keys', dict(res=112, keys=5, out_mode=OUT_F32), dict(form=SPLIT, tws=128, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('u8 116 5 keys', dict(res=116, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=128, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 116 5 keys', dict(res=116, keys=5, out_mode=OUT_F32), dict(form=SPLIT, tws=128, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('u8 120 5 keys', dict(res=120, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=128, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 120 5 keys', dict(res=120, keys=5, out_mode=OUT_F32), dict(form=BITS, twp=128, strips=1, nwv=4, nb=3, minwg=4, emit=0, persist=0, grid=65536)),
    ('u8 128 5 keys', dict(res=128, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=128, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 128 5 keys', dict(res=128, keys=5, out_mode=OUT_F32), dict(form=SPLIT, tws=128, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('u8 144 5 keys', dict(res=144, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=160, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 144 5 keys', dict(res=144, keys=5, out_mode=OUT_F32), dict(form=SPLIT, tws=160, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('u8 160 5 keys', dict(res=160, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=160, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 160 5 keys', dict(res=160, keys=5, out_mode=OUT_F32), dict(form=SPLIT, tws=160, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('u8 208 5 keys', dict(res=208, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=224, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 208 5 keys', dict(res=208, keys=5, out_mode=OUT_F32), dict(form=BITS, twp=224, strips=1, nwv=4, nb=3, minwg=4, emit=0, persist=0, grid=65536)),
    ('u8 216 5 keys', dict(res=216, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=224, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('f32 216 5 keys', dict(res=216, keys=5, out_mode=OUT_F32), dict(form=BITS, twp=224, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('u8 224 5 keys', dict(res=224, keys=5, out_mode=OUT_U8), dict(form=BITS, twp=224, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('f32 224 5 keys', dict(res=224, keys=5, out_mode=OUT_F32), dict(form=BITS, twp=224, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('u8 320 5 keys', dict(res=320, keys=5, out_mode=OUT_U8), dict(form=BITS, twp=160, strips=2, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('f32 320 5 keys', dict(res=320, keys=5, out_mode=OUT_F32), dict(form=BITS, twp=160, strips=2, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('u8 512 5 keys', dict(res=512, keys=5, out_mode=OUT_U8), dict(form=BITS, twp=128, strips=4, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('f32 512 5 keys', dict(res=512, keys=5, out_mode=OUT_F32), dict(form=BITS, twp=128, strips=4, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('narrowed: u8 160 10 keys, K3r over the LDS budget', dict(res=160, keys=10, out_mode=OUT_U8), dict(form=BITS, twp=160, strips=1, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=768)),
    ('not narrowed below 160: u8 144 10 keys', dict(res=144, keys=10, out_mode=OUT_U8), dict(form=SPLIT, tws=128, lw=4, caps=1636, nb=4, persist=1, grid=512)),
    ('K3r 2 waves: f32 96', dict(res=96, keys=5), dict(form=SPLIT, tws=96, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('K3r 4 waves: f32 100', dict(res=100, keys=5), dict(form=SPLIT, tws=128, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('K3r 2 waves: u8 128', dict(res=128, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=128, lw=2, caps=1636, nb=3, persist=1, grid=512)),
    ('K3r 4 waves: u8 144', dict(res=144, keys=5, out_mode=OUT_U8), dict(form=SPLIT, tws=160, lw=4, caps=1636, nb=3, persist=1, grid=512)),
    ('index slices: EMIT, 4 waves', dict(res=256, keys=5, slices=True), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=1, persist=1, grid=768)),
    ('index slices: 4 waves, never 8 (6 keys)', dict(res=256, keys=6, slices=True), dict(form=BITS, twp=128, strips=2, nwv=4, nb=3, minwg=3, emit=1, persist=1, grid=768)),
    ('index slices: no split form', dict(res=128, keys=5, slices=True), dict(form=BITS, twp=128, strips=1, nwv=4, nb=3, minwg=3, emit=1, persist=1, grid=768)),
    ('index slices with 8 waves: ELIMIT', dict(res=256, keys=5, slices=True, bits_waves=8), dict(form=ELIMIT)),
    ('index slices with 16+ keys: ELIMIT', dict(res=256, keys=-1, slices=True), dict(form=ELIMIT)),
    ('no workspace: one workgroup per item', dict(res=256, keys=5, ws=0), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=0, grid=65536)),
    ('no workspace: no split form', dict(res=128, keys=5, out_mode=OUT_U8, ws=0), dict(form=BITS, twp=128, strips=1, nwv=4, nb=3, minwg=4, emit=0, persist=0, grid=65536)),
    ('workspace for 127 records: no split form', dict(res=128, keys=5, out_mode=OUT_U8, ws=166986112), dict(form=BITS, twp=128, strips=1, nwv=4, nb=3, minwg=4, emit=0, persist=0, grid=65536)),
    ('workspace for 128 records: split form', dict(res=128, keys=5, out_mode=OUT_U8, ws=168296832), dict(form=SPLIT, tws=128, lw=2, caps=128, nb=3, persist=1, grid=512)),
    ('advisor: u8 192 8 keys', dict(res=192, keys=8, out_mode=OUT_U8), dict(form=BITS, twp=192, strips=1, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=768)),
    ('advisor: u8 192 9 keys', dict(res=192, keys=9, out_mode=OUT_U8), dict(form=BITS, twp=192, strips=1, nwv=8, nb=4, minwg=0, emit=0, persist=0, grid=65536)),
    ('advisor: u8 192 10 keys', dict(res=192, keys=10, out_mode=OUT_U8), dict(form=BITS, twp=192, strips=1, nwv=8, nb=4, minwg=0, emit=0, persist=0, grid=65536)),
    ('advisor: u8 208 8 keys', dict(res=208, keys=8, out_mode=OUT_U8), dict(form=BITS, twp=224, strips=1, nwv=8, nb=4, minwg=0, emit=0, persist=0, grid=65536)),
    ('advisor: u8 208 9 keys', dict(res=208, keys=9, out_mode=OUT_U8), dict(form=BITS, twp=224, strips=1, nwv=8, nb=4, minwg=0, emit=0, persist=0, grid=65536)),
    ('advisor: u8 208 10 keys', dict(res=208, keys=10, out_mode=OUT_U8), dict(form=BITS, twp=224, strips=1, nwv=8, nb=4, minwg=0, emit=0, persist=0, grid=65536)),
    ('advisor: u8 216 8 keys', dict(res=216, keys=8, out_mode=OUT_U8), dict(form=BITS, twp=224, strips=1, nwv=8, nb=4, minwg=0, emit=0, persist=0, grid=65536)),
    ('advisor: u8 216 9 keys', dict(res=216, keys=9, out_mode=OUT_U8), dict(form=BITS, twp=224, strips=1, nwv=8, nb=4, minwg=0, emit=0, persist=0, grid=65536)),
    ('advisor: u8 216 10 keys', dict(res=216, keys=10, out_mode=OUT_U8), dict(form=BITS, twp=128, strips=2, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=768)),
    ('NO_SPLIT', dict(res=128, keys=5, out_mode=OUT_U8, debug=D.NO_SPLIT), dict(form=BITS, twp=128, strips=1, nwv=4, nb=3, minwg=4, emit=0, persist=0, grid=65536)),
    ('SPLIT at 256', dict(res=256, keys=5, out_mode=OUT_U8, debug=D.SPLIT), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=768)),
    ('WHOLE_4WAVES', dict(res=256, keys=6, debug=D.WHOLE_4WAVES), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=512)),
    ('NO_8WAVES', dict(res=256, keys=6, debug=D.NO_8WAVES), dict(form=BITS, twp=128, strips=2, nwv=4, nb=3, minwg=4, emit=0, persist=0, grid=131072)),
    ('WIDEST_STRIPS', dict(res=256, keys=9, debug=D.WIDEST_STRIPS), dict(form=BITS, twp=224, strips=2, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=512)),
    ('NO_EXTRA_STRIP', dict(res=256, keys=10, debug=D.NO_EXTRA_STRIP), dict(form=BITS, twp=128, strips=2, nwv=4, nb=4, minwg=3, emit=0, persist=1, grid=512)),
    ('MINWG3', dict(res=256, keys=3, debug=D.MINWG3), dict(form=BITS, twp=256, strips=1, nwv=4, nb=2, minwg=3, emit=0, persist=1, grid=768)),
    ('GRID8', dict(res=256, keys=5, debug=D.GRID8), dict(form=BITS, twp=256, strips=1, nwv=4, nb=3, minwg=3, emit=0, persist=1, grid=2048)),
    ('NO_BITS', dict(res=256, keys=5, debug=D.NO_BITS), dict(form=FUSED, tw=64, strips=4, grid=262144)),
    ('NO_BINNED', dict(res=256, keys=-1, debug=D.NO_BINNED), dict(form=FUSED, tw=64, strips=4, grid=262144)),
]


@pytest.mark.parametrize('call,expected', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_plan(call, expected):
    _native.build()
    got = plan(**call)
    assert {k: got[k] for k in expected} == expected


def test_split_form_workspace_layout():
    """the split form's workspace: markers at 0, counts and 16-byte records 256-aligned, the 4-byte fourth words after the records.  The
    recommended workspace counts LIST_CAPS = 2048 records of 16 bytes, the launch divides by 20: 1636 records per camera, kept as measured."""
    _native.build()
    n = 4096
    p = plan(128, 5, OUT_U8, n_img=n)
    assert p['form'] == SPLIT
    assert p['off_counts'] == ((n + 1) * 4 + 255) // 256 * 256
    assert p['off_lists'] == p['off_counts'] + (n * 4 + 255) // 256 * 256
    assert p['caps'] == (2048 * 16 // 20) & ~3 == 1636
    assert p['off_lists3'] == p['off_lists'] + n * p['caps'] * 16
    assert p['off_lists3'] + n * p['caps'] * 4 <= workspace(n, 128, OUT_U8, 5) - 64
