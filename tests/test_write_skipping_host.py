"""The host side of write skipping, without a GPU: when a render into an owned buffer may leave background lines alone
(_ops.write_skip_decision: plain values in, one of three answers out) and that the ring probe of rendering.allocate_image_ring keeps timing
full writes (_DeviceTimer forgets the buffer's coverage before every timed render)."""
import ctypes

import torch

from torchdrivesim_amd import _native as nat
from torchdrivesim_amd import _ops
from torchdrivesim_amd.rendering import hip


def decide(record='valid', whole=True, res=256, n_img=12, version=3, capturing=False, enabled=True):
    if record == 'valid':
        record = dict(res=256, n_img=12, version=3, valid=True)
    return _ops.write_skip_decision(record, whole, res, n_img, version, capturing, enabled)


def test_lines_are_skipped_only_when_everything_holds():
    assert decide() == 'skip'
    # no record yet, a record the last call did not maintain, another resolution or camera count, a write torch has seen, the switch: store everything, record it
    assert decide(record=None) == 'rewrite'
    assert decide(record=dict(res=256, n_img=12, version=3, valid=False)) == 'rewrite'
    assert decide(record=dict(res=192, n_img=12, version=3, valid=True), res=192, n_img=24) == 'rewrite'
    assert decide(record=dict(res=128, n_img=12, version=3, valid=True)) == 'rewrite'
    assert decide(version=4) == 'rewrite'
    assert decide(enabled=False) == 'rewrite'
    # part of a buffer (or another shape over it), a side that is no multiple of 32, no version counter, stream capture: no record at all
    assert decide(whole=False) == 'untracked'
    assert decide(res=200, record=None) == 'untracked'
    assert decide(version=_ops._NO_VERSION) == 'untracked'
    assert decide(capturing=True) == 'untracked'
    assert decide(capturing=True, enabled=False) == 'untracked' and decide(whole=False, record=None) == 'untracked'


def test_the_switches_exist_and_default_to_on():
    assert _ops.use_write_skipping is True
    assert hip.HipRendererConfig().write_skipping is True and hip.HipRendererConfig(write_skipping=False).write_skipping is False


def test_forgetting_a_tensor_that_is_no_owned_buffer_is_harmless():
    _ops.forget_coverage(torch.zeros(4))
    _ops.forget_coverage(None)


def test_the_aux_struct_matches_the_header_and_the_size_query_counts_lines():
    assert ctypes.sizeof(nat.RasterAux) == 112 and nat.RasterAux.coverage.offset == 96 and nat.RasterAux.coverage_maintained.offset == 92
    assert nat.RASTER_REWRITE_ALL == 2
    n = ctypes.c_int64(-1)
    L = nat.lib()
    assert L.tds_raster_coverage_bytes(65536, 256, ctypes.byref(n)) == 0 and n.value == 64 + 65536 * 256      # res^2 / 256 bytes per camera
    assert L.tds_raster_coverage_bytes(12, 192, ctypes.byref(n)) == 0 and n.value == 64 + 12 * 36 * 4
    assert L.tds_raster_coverage_bytes(12, 200, ctypes.byref(n)) == 0 and n.value == 0                        # no lines to track
    assert L.tds_raster_coverage_bytes(12, 0, ctypes.byref(n)) == nat.E_INVAL


def test_the_ring_probe_forgets_the_coverage_before_every_timed_render(monkeypatch):
    log = []
    monkeypatch.setattr(_ops, 'forget_coverage', lambda buf: log.append(('forget', buf)))
    timer = hip._DeviceTimer(lambda buf: log.append(('render', buf)), torch.device('cpu'), reps=3)
    monkeypatch.setattr(timer, '_ms', lambda fn, reps: [fn() or 1.0 for _ in range(reps)])       # (the real one brackets fn with device events)
    buf = object()
    assert timer.first_touch(buf) == 1.0
    assert log == [('forget', buf), ('render', buf)]
    del log[:]
    assert timer.launch(buf) == 1.0
    assert log == [('forget', buf), ('render', buf)] * 3
