"""Semantic bird's-eye masks (tds_raster_scene_masks, Simulator.render_semantic) on the CPU: the exported symbols, the launch plan of the mask
modes, the channel specification, the packed-bit helper and the register budget of the mask kernels.  The pixels are checked on the GPU
(tests/test_gpu_semantic_masks.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from torchdrivesim_amd import _native
from torchdrivesim_amd._native import OUT_MASK_BITS, OUT_MASK_U8, OUT_U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_mask_entry_points_are_exported():
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _native.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {'tds_raster_scene_masks', 'tds_raster_scene_masks_multi'} <= names
    L = _native.lib()
    assert L.tds_raster_scene_masks.argtypes is not None and L.tds_raster_scene_masks_multi.argtypes is not None


def _ws(n_img, res, mode, keys):
    n = ctypes.c_int64()
    _native.check(_native.lib().tds_raster_scene_workspace_bytes_for(n_img, res, mode, keys, ctypes.byref(n)), 'workspace_bytes_for')
    return n.value


def test_mask_workspace_is_the_uint8_one_plus_the_channel_table():
    for n_img, res, keys in ((65536, 256, 5), (65536, 128, 7), (512, 64, 3), (7, 31, 15), (100, 216, -1)):
        for mode in (OUT_MASK_U8, OUT_MASK_BITS):
            assert _ws(n_img, res, mode, keys) == _ws(n_img, res, OUT_U8, keys) + 256


def test_mask_modes_take_the_uint8_plan():
    """every shape of tests/test_raster_plan.py: the mask modes plan as the uint8 image (workspace: what the product recommends for the mode),
    minus the pair table's LDS; shapes the uint8 image would give to the packed-key kernels are TDS_ELIMIT for the masks"""
    import test_raster_plan as trp
    checked = 0
    for name, call, _ in trp.CASES:
        call = dict(call)
        if call.get('slices'):
            continue
        call['out_mode'] = OUT_U8
        u8 = trp.plan(**call)
        for mode in (OUT_MASK_U8, OUT_MASK_BITS):
            m = trp.plan(**dict(call, out_mode=mode, ws=call.get('ws', None) if call.get('ws', None) is None or call['ws'] == 0 else call['ws'] + 256))
            if u8['form'] in (trp.BITS, trp.SPLIT):
                tab = 3 * (1 << (2 * u8['nb'])) * 4
                assert {k: v for k, v in m.items() if k not in ('lds', 'lds_s')} == {k: v for k, v in u8.items() if k not in ('lds', 'lds_s')}, name
                assert m['lds'] == u8['lds'] - tab, name
                assert m['lds_s'] == (u8['lds_s'] - tab if u8['form'] == trp.SPLIT else u8['lds_s']), name
            elif u8['form'] != trp.ELIMIT:
                assert m['form'] == trp.ELIMIT, name
            checked += 1
    assert checked > 100


# ---- channel specification (host logic of Simulator.render_semantic, on a stand-in scene) ---------------------------------------------
class _Map:
    """what the channel logic reads of a scene's map: its level table and its face keys"""

    def __init__(self, levels, face_keys):
        self.levels, self._keys = [float(v) for v in levels], face_keys

    def rank_of(self, level):
        return self.levels.index(float(level)) + 1

    def face_keys(self):
        return self._keys


def _sim(agent_types=('vehicle',), controls=(), waypoints=False, color_map=None):
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.rendering import HipRenderer, HipRendererConfig
    from torchdrivesim_amd.rendering.hip import level_table
    from torchdrivesim_amd.simulator import Simulator
    r = HipRenderer(HipRendererConfig(), color_map=color_map)
    lv, cm = r.rendering_levels, r.color_map
    actor = list(agent_types) + ['direction', 'goal_waypoint'] + list(controls)
    levels = level_table([lv[c] for c in ('road', 'left_lane', 'right_lane')], [lv[c] for c in actor])
    m = _Map(levels, [])
    key = lambda n: (m.rank_of(lv[n]) << 24) | int(_ops.quantise_colors(torch.tensor(cm[n], dtype=torch.float32) / 255.0))  # noqa: E731
    m._keys = [key(c) for c in ('road', 'left_lane', 'right_lane')]
    scene = dict(map=m, key_table=sorted({key(n) for n in list(agent_types) + ['direction'] + list(controls)}), wp_key=key('goal_waypoint'))
    sim = object.__new__(Simulator)
    sim.renderer, sim.waypoint_goals = r, (object() if waypoints else None)
    sim._scene = lambda: scene
    return sim, scene, key


def test_default_channels_follow_the_rendering_levels():
    sim, scene, _ = _sim(agent_types=('vehicle', 'pedestrian', 'bicycle'))
    assert sim.semantic_channels() == ['road', 'right_lane', 'left_lane', 'pedestrian', 'bicycle', 'vehicle', 'direction']
    assert sim.semantic_channels() == sim.semantic_channels()
    sim, scene, _ = _sim(controls=('traffic_light_green', 'traffic_light_red', 'traffic_light_yellow', 'stop_sign'), waypoints=True)
    assert sim.semantic_channels() == ['road', 'right_lane', 'left_lane', 'stop_sign', 'traffic_light_green', 'traffic_light_red',
                                       'traffic_light_yellow', 'goal_waypoint', 'vehicle', 'direction']


def test_channels_are_unions_and_absent_categories_are_zero():
    sim, scene, key = _sim(agent_types=('vehicle',))
    chans, kc = sim._semantic_spec(scene, [('road', 'left_lane', 'right_lane'), 'vehicle', ['pedestrian', 'bicycle'], 'direction', 'road'])
    assert chans == [('road', 'left_lane', 'right_lane'), ('vehicle',), ('pedestrian', 'bicycle'), ('direction',), ('road',)]
    assert kc[key('road')] == 0b10001 and kc[key('left_lane')] == 0b1 and kc[key('right_lane')] == 0b1
    assert kc[key('vehicle')] == 0b10 and kc[key('direction')] == 0b1000
    # pedestrian / bicycle have keys (their levels are in the table here) but no face of this scene carries them: the channel stays zero
    assert not any(v & 0b100 for k, v in kc.items() if k in set(scene['map'].face_keys()) | set(scene['key_table']))
    # a category whose level the scene never draws at has no key at all
    assert 'prediction' not in sim._category_keys(scene)
    chans, kc = sim._semantic_spec(scene, ['prediction', 'road'])
    assert set(kc) == {key('road')} and kc[key('road')] == 0b10


def test_unknown_names_shared_keys_and_too_many_channels_are_refused():
    sim, scene, _ = _sim()
    with pytest.raises(ValueError, match='unknown category'):
        sim._semantic_spec(scene, ['road', 'sidewalk'])
    with pytest.raises(ValueError, match='unknown category'):
        sim._semantic_spec(scene, ['background'])
    with pytest.raises(ValueError, match='1 to 32'):
        sim._semantic_spec(scene, ['road'] * 33)
    with pytest.raises(ValueError, match='1 to 32'):
        sim._semantic_spec(scene, [])
    assert len(sim._semantic_spec(scene, ['road'] * 32)[0]) == 32
    # two categories with the same colour and level: naming one without the other is ambiguous
    from torchdrivesim_amd.rendering import get_default_color_map
    cm = get_default_color_map()
    cm['stop_sign'] = cm['yield_sign']
    sim, scene, _ = _sim(controls=('stop_sign', 'yield_sign'), color_map=cm)
    with pytest.raises(ValueError, match="'stop_sign'.*'yield_sign'"):
        sim._semantic_spec(scene, ['stop_sign'])
    chans, kc = sim._semantic_spec(scene, [('stop_sign', 'yield_sign')])
    assert list(kc.values()) == [1]


def test_non_hip_renderers_refuse():
    from torchdrivesim_amd.rendering import DummyRenderer, DummyRendererConfig
    sim, _, _ = _sim()
    sim.renderer = DummyRenderer(DummyRendererConfig())
    with pytest.raises(NotImplementedError):
        sim.render_semantic(torch.zeros(1, 1, 2), torch.zeros(1, 1, 1))
    with pytest.raises(NotImplementedError):
        sim.semantic_channels()


@pytest.mark.parametrize('res', [1, 4, 31, 32, 33, 64, 100, 256])
def test_unpack_mask_bits_matches_numpy(res):
    from torchdrivesim_amd.rendering import unpack_mask_bits
    rng = np.random.default_rng(res)
    wpw = (res + 31) // 32
    words = rng.integers(0, 2 ** 32, size=(2, 3, 4, wpw, res), dtype=np.uint64).astype(np.uint32)
    got = unpack_mask_bits(torch.from_numpy(words.view(np.int32)), res)
    assert got.dtype == torch.bool and tuple(got.shape) == (2, 3, 4, res, res)
    ref = np.unpackbits(words.view(np.uint8).reshape(2, 3, 4, wpw, res, 4), axis=-1, bitorder='little')    # (..., xw, y, 32)
    ref = np.moveaxis(ref, -1, -2).reshape(2, 3, 4, wpw * 32, res)[..., :res, :].astype(bool)
    np.testing.assert_array_equal(got.numpy(), ref)
    with pytest.raises(ValueError):
        unpack_mask_bits(torch.from_numpy(words.view(np.int32))[..., :-1], res)


def test_mask_kernels_stay_within_the_uint8_budgets():
    """Every mask instantiation of the bit-plane kernels next to its uint8 colour counterpart (same waves, index bits, arguments, occupancy).
    As built here (ROCm 6 / gfx950): K3r and the 8-wave / MINWG = 4 kernels spill exactly as their uint8 twins or less; the persistent
    MINWG = 3 kernels keep three waves per SIMD at 64 - 80 bytes of scratch per lane -- one of them, <4, 2, MaskU8, SceneArgs, false, 3>, at 80
    where its uint8 twin has 64, still within the 80 bytes the colour kernels are held to (tests/test_kernel_resources.py)."""
    import kernel_resources
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    t = kernel_resources.kernel_table(_native.LIB_PATH)
    masks = {k: v for k, v in t.items() if re.search(r'<.*Mask(U8|Bits)', k)}
    assert len(masks) == 2 * (3 * 2 + 3 * 2 * 2 + 3), sorted(masks)        # K3r: nb x waves; 4 waves: nb x args x minwg; 8 waves: nb
    for name, e in masks.items():
        twin = t[re.sub(r'Mask(U8|Bits)', 'unsigned char', name)]
        assert e['waves_per_simd'] >= twin['waves_per_simd'], (name, e, twin)
        budget = max(twin['private_segment_fixed_size'], 80 if name.endswith('false, 3>') and name.startswith('raster_scene_bits_kernel<4') else 0)
        assert e['private_segment_fixed_size'] <= budget, (name, e, twin)
        if name.startswith('raster_list_bits_kernel'):
            assert e['private_segment_fixed_size'] == 0 and e['vgpr_spill_count'] == 0, (name, e)
