"""The host side of the prepared scan set-ups (include/tdship.h, tds_raster_aux_t::camera_prep): how large the table is.  One record of 336 bytes
(the camera and its trim polygon, the grid window, sixteen grid rows) per work item -- camera and strip -- of the launch that takes the table, the
persistent bit-plane launch; nothing where another launch serves the shape.  No GPU involved: the sizing function asks the launch plan."""
import ctypes

import pytest

from torchdrivesim_amd import _native as nat

RECORD = 336


@pytest.fixture(scope='module')
def L():
    return nat.lib()


def prep_bytes(L, n_img, res, mode, n_keys):
    n = ctypes.c_int64(-1)
    assert L.tds_raster_camera_prep_bytes(n_img, res, mode, n_keys, ctypes.byref(n)) == 0
    return n.value


def test_one_record_per_camera_and_monotone_in_the_cameras(L):
    sizes = [prep_bytes(L, n, 256, nat.OUT_F32, 5) for n in (0, 1, 2, 16, 17, 4096, 65536)]
    assert sizes == [n * RECORD for n in (0, 1, 2, 16, 17, 4096, 65536)]
    assert sizes == sorted(sizes)
    assert prep_bytes(L, 65536, 256, nat.OUT_U8, 5) == 65536 * RECORD


def test_strips_are_accounted_for(L):
    # nine keys at 256 x 256: two strips of 128 columns, each a work item of its own (tests/test_raster_plan.py pins the plan)
    assert prep_bytes(L, 16, 256, nat.OUT_F32, 9) == 2 * 16 * RECORD
    # six keys: the plain call takes the whole image in 8-wave workgroups (no table), the differentiable call two half-image strips in 4-wave
    # ones -- the table is sized for the larger of the two
    assert prep_bytes(L, 16, 256, nat.OUT_F32, 6) == 2 * 16 * RECORD
    assert prep_bytes(L, 16, 256, nat.OUT_U8, 6) == 0


def test_shapes_that_another_launch_serves_need_no_table(L):
    assert prep_bytes(L, 16, 192, nat.OUT_U8, 5) == 0           # four workgroups per CU: one item per workgroup, no table
    assert prep_bytes(L, 16, 192, nat.OUT_F32, 5) == 16 * RECORD    # (float32: the differentiable call of that shape is a persistent launch)
    assert prep_bytes(L, 16, 128, nat.OUT_U8, 5) == 0           # the split form (the fused launch over overflowed cameras takes none)
    assert prep_bytes(L, 16, 256, nat.OUT_F32, -1) == 0         # keys not known: packed keys
    assert prep_bytes(L, 16, 256, nat.OUT_MASK_U8, 5) == 0      # the masks take no table


def test_bad_arguments_are_refused_by_code(L):
    n = ctypes.c_int64(7)
    for args in ((-1, 256, nat.OUT_F32, 5), (1 << 31, 256, nat.OUT_F32, 5), (16, 0, nat.OUT_F32, 5), (16, 4097, nat.OUT_F32, 5), (16, 256, 9, 5),
                 (16, 256, -1, 5), (16, 256, nat.OUT_F32, 16), (16, 256, nat.OUT_F32, -2)):
        assert L.tds_raster_camera_prep_bytes(*args, ctypes.byref(n)) == nat.E_INVAL, args
        assert n.value == 0
    assert L.tds_raster_camera_prep_bytes(16, 256, nat.OUT_F32, 5, None) == nat.E_INVAL


def test_the_aux_struct_ends_with_the_table(L):
    """tds_raster_aux_t: the two new fields are appended, and read only under TDS_RASTER_HAS_CAMERA_PREP -- the struct that ends with coverage_bytes
    (nat.RasterAux, what a caller built against the older header passes) stays as it was and stays valid"""
    import re
    from pathlib import Path
    assert [f[0] for f in nat.RasterAux._fields_][-2:] == ['coverage', 'coverage_bytes'] and ctypes.sizeof(nat.RasterAux) == 112
    assert [f[0] for f in nat.RasterAuxPrep._fields_] == ['camera_prep', 'camera_prep_bytes'] and issubclass(nat.RasterAuxPrep, nat.RasterAux)
    assert nat.RasterAuxPrep.camera_prep.offset == 112 and nat.RasterAuxPrep.camera_prep_bytes.offset == 120 and ctypes.sizeof(nat.RasterAuxPrep) == 128
    header = (Path(__file__).resolve().parents[1] / 'include' / 'tdship.h').read_text()
    body = re.search(r'typedef struct tds_raster_aux \{(.*?)\} tds_raster_aux_t;', header, re.S).group(1)
    members = re.findall(r'(\w+)(?:\[\d+\])?;', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert members == [f[0] for f in nat.RasterAux._fields_] + [f[0] for f in nat.RasterAuxPrep._fields_]
    assert int(re.search(r'#define TDS_RASTER_HAS_CAMERA_PREP (\d+)', header).group(1)) == nat.RASTER_HAS_CAMERA_PREP == 4


def test_the_python_side_asks_for_no_table_where_the_keys_rule_out_the_bit_planes(monkeypatch):
    """_ops sizes a table only for 1 .. 15 keys (more, or an unknown number: packed keys); the switches exist and default to on"""
    from torchdrivesim_amd import _ops
    from torchdrivesim_amd.rendering import hip
    monkeypatch.setattr(_ops.nat, 'call', lambda *a, **k: pytest.fail('no call expected'))
    for n_keys in (-1, 0, 16, 40):
        assert _ops._camera_prep_table(None, 16, 256, nat.OUT_F32, n_keys) is None
    assert _ops.use_camera_prep is True
    assert hip.HipRendererConfig().camera_prep is True and hip.HipRendererConfig(camera_prep=False).camera_prep is False
