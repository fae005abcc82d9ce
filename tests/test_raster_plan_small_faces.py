"""Which launches paint small faces on the lane that scanned them (tds_raster_plan.h: RasterPlan::small_lane, through the testing hook
tds_raster_plan_small_lane; CPU only).  Over the whole plan sweep of tests/test_raster_plan.py the path is on exactly for the 4-wave bit-plane
instantiations at three workgroups per CU (the ones that have the block, raster.hip: SROWS), and only while the caller allows it
(HipRendererConfig.small_faces / _ops.use_small_faces -> TDS_RASTER_NO_SMALL_FACES); never for the 8-wave and the four-per-CU instantiations,
the packed-key forms or the masks."""
import ctypes

import pytest

from test_raster_plan import BITS, CASES, SPLIT, plan, workspace
from torchdrivesim_amd import _native
from torchdrivesim_amd._native import OUT_F32, OUT_MASK_BITS, OUT_MASK_U8, OUT_U8


def small_lane(res, keys, out_mode=OUT_F32, n_img=65536, listed=True, actors=True, extra=False, slices=False, ws=None, cus=256,
               force_tw=0, bits_waves=4, list_waves=0, list_lds_kb=40, debug=0, small_faces=True):
    if ws is None:
        ws = workspace(n_img, res, out_mode, keys)
    out = ctypes.c_int(-1)
    _native.check(_native.testing_lib().tds_raster_plan_small_lane(n_img, res, out_mode, keys, int(listed), int(actors), int(extra), int(slices), ws, cus, force_tw,
                                                                   bits_waves, list_waves, list_lds_kb, int(debug), int(small_faces), ctypes.byref(out)),
                  'tds_raster_plan_small_lane')
    return out.value


@pytest.mark.parametrize('call', [c[1] for c in CASES], ids=[c[0] for c in CASES])
def test_the_path_is_on_exactly_for_the_4_wave_three_per_cu_forms(call):
    _native.build()
    p = plan(**call)
    has_block = p['form'] in (BITS, SPLIT) and p['nwv'] == 4 and p['minwg'] == 3
    assert small_lane(**call) == int(has_block)
    assert small_lane(**call, small_faces=False) == 0


def test_the_sweep_holds_both_kinds():
    _native.build()
    on = [c[0] for c in CASES if small_lane(**c[1])]
    off = [c[0] for c in CASES if not small_lane(**c[1])]
    assert 'headline f32 256 5 keys' in on and 'index slices: EMIT, 4 waves' in on and 'u8 256 8 keys' in on and 'no workspace: one workgroup per item' in on
    for name in ('f32 256 3 keys', 'f32 256 6 keys', 'u8 256 7 keys', '16+ keys, workspace: binned', 'actor keys not listed: fused', 'f32 208 5 keys', 'NO_BITS'):
        assert name in off, name


@pytest.mark.parametrize('mode', [OUT_MASK_U8, OUT_MASK_BITS])
def test_the_masks_never_take_it(mode):
    _native.build()
    assert small_lane(256, 5, mode) == 0
    assert small_lane(256, 5, OUT_U8) == 1
