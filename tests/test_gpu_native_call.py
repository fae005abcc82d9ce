"""_native.call marshals its arguments from the declaration of the entry point (torchdrivesim_amd/_native.py): tensors are checked and become
pointers, raw ctypes pointers pass through, an omitted stream is torch's current one.  Two boxes through tds_box2corners_f32."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def two_boxes():
    box = torch.tensor([[1.0, 2.0, 4.5, 2.0, 0.3], [-3.0, 0.5, 5.0, 2.2, 2.0]], device=DEV)
    sc = torch.stack([torch.sin(box[:, 4]), torch.cos(box[:, 4])], dim=-1).contiguous()
    return box, sc


def corners_of(*args, on=None):
    """the call's output for these arguments (... = the output tensor); `on`: the side stream it is given, which waits for the output's fill"""
    from torchdrivesim_amd import _native as nat
    out = torch.full((2, 4, 2), float('nan'), device=DEV)
    if on is not None:
        on.wait_stream(torch.cuda.current_stream(DEV))
    nat.call('tds_box2corners_f32', DEV, *[out if a is Ellipsis else a for a in args])
    torch.cuda.synchronize()
    return out


def test_a_wrong_dtype_and_a_view_are_refused_by_name_and_nothing_is_launched():
    from torchdrivesim_amd import _native as nat
    box, sc = two_boxes()
    out = torch.full((2, 4, 2), -7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r'^sc: expected torch.float32, got torch.float64'):
        nat.call('tds_box2corners_f32', DEV, box, sc.double(), out, 2)
    wide = torch.zeros(2, 10, device=DEV)
    wide[:, ::2] = box
    assert torch.equal(wide[:, ::2], box) and not wide[:, ::2].is_contiguous()
    with pytest.raises(RuntimeError, match=r'^box: tensor must be contiguous'):
        nat.call('tds_box2corners_f32', DEV, wide[:, ::2], sc, out, 2)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), 'a refused call wrote its output'


def test_raw_pointers_give_the_same_bits_as_tensors():
    from torchdrivesim_amd import _native as nat
    box, sc = two_boxes()
    by_tensor = corners_of(box, sc, ..., 2)
    assert bool(torch.isfinite(by_tensor).all()) and torch.allclose(by_tensor.mean(dim=1), box[:, :2], atol=1e-5)      # (it ran: centred on the boxes)
    raw = torch.full((2, 4, 2), float('nan'), device=DEV)
    nat.call('tds_box2corners_f32', DEV, ctypes.c_void_p(box.data_ptr()), nat.dev_ptr(sc, torch.float32, 'sc'), raw.data_ptr(), ctypes.c_int64(2),
             nat.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert torch.equal(raw, by_tensor)


def test_an_omitted_stream_is_the_current_stream():
    box, sc = two_boxes()
    want = corners_of(box, sc, ..., 2)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        omitted = corners_of(box, sc, ..., 2)
    as_stream, as_pointer = corners_of(box, sc, ..., 2, s, on=s), corners_of(box, sc, ..., 2, ctypes.c_void_p(s.cuda_stream), on=s)
    assert torch.equal(omitted, want) and torch.equal(as_stream, want) and torch.equal(as_pointer, want)
