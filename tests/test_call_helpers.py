"""The wrappers' shared helpers (camouflage_multimodal_amd/_lib.py) on the CPU: a stand-in object takes the loaded library's place,
so neither the shared library nor a device is needed."""
import pytest
import torch

from camouflage_multimodal_amd import _lib


class _StandIn:
    """What ``_lib.lib()`` returns, reduced to two bytes functions and the last error."""

    def __init__(self):
        self.asked = []

    def camo_none_workspace_bytes(self, *args):
        self.asked.append(args)
        return 0

    def camo_some_workspace_bytes(self, *args):
        self.asked.append(args)
        return 48

    def camo_last_error(self):
        return b"the stand-in's words"


@pytest.fixture
def stand_in(monkeypatch):
    s = _StandIn()
    monkeypatch.setattr(_lib, "_lib", s)                      # (lib() returns what is loaded; the real binding comes back afterwards)
    return s


def test_workspace_refuses_with_the_call_sites_exception(stand_in):
    with pytest.raises(ValueError, match=r"^camo_instances does not support N = 2, H = 3, W = 4$"):
        _lib.workspace("camo_none_workspace_bytes", 2, 3, 4, device="cpu", refuse=lambda: ValueError("camo_instances does not support N = 2, H = 3, W = 4"))
    with pytest.raises(_lib.CamoError, match=r"^camo_seg_weighted_f does not support N = 2, H = 3, W = 4$") as e:
        _lib.workspace("camo_none_workspace_bytes", 2, 3, 4, device="cpu",
                        refuse=lambda: _lib.CamoError("camo_seg_weighted_f does not support N = 2, H = 3, W = 4"))
    assert type(e.value) is _lib.CamoError
    # the region-graph callers: the library's own words through check(-1, ..)
    with pytest.raises(_lib.CamoError, match=r"^camo_none_workspace_bytes failed \(code -1\): the stand-in's words$"):
        _lib.workspace("camo_none_workspace_bytes", 2, 3, 4, device="cpu")
    assert stand_in.asked == [(2, 3, 4)] * 3


def test_workspace_where_zero_is_valid(stand_in):
    ws, need = _lib.workspace("camo_none_workspace_bytes", 2, 3, 4, 3, 0, device="cpu", refuse=False)
    assert need == 0 and ws.dtype == torch.uint8 and ws.numel() == 1          # the true size for the library, a buffer it can point at
    assert stand_in.asked == [(2, 3, 4, 3, 0)]


def test_workspace_allocates_what_the_library_states(stand_in):
    for refuse in (None, False, lambda: ValueError("not raised")):
        ws, need = _lib.workspace("camo_some_workspace_bytes", 7, device="cpu", refuse=refuse)
        assert need == 48 and ws.dtype == torch.uint8 and tuple(ws.shape) == (48,) and ws.device.type == "cpu"


def test_label_map():
    t = torch.zeros(3, 4, dtype=torch.int32)
    got = _lib.label_map(t, "labels")
    assert tuple(got.shape) == (1, 3, 4) and got.data_ptr() == t.data_ptr()
    b = torch.zeros(2, 3, 4, dtype=torch.int32)
    assert _lib.label_map(b, "labels") is b
    with pytest.raises(ValueError, match=r"^gt_labels must be int32, got torch\.int64$"):
        _lib.label_map(torch.zeros(2, 3, 4, dtype=torch.int64), "gt_labels")
    with pytest.raises(ValueError, match=r"^need labels \[N, H, W\] or \[H, W\] with at least one pixel, got \(2, 0, 4\)$"):
        _lib.label_map(torch.zeros(2, 0, 4, dtype=torch.int32), "labels")
    with pytest.raises(ValueError, match=r"^need labels \[N, H, W\] or \[H, W\] with at least one pixel, got \(1, 2, 3, 4\)$"):
        _lib.label_map(torch.zeros(1, 2, 3, 4, dtype=torch.int32), "labels")
    with pytest.raises(ValueError, match=r"^pred_boundary must be a tensor$"):
        _lib.label_map([[0, 1]], "pred_boundary")
    with pytest.raises(ValueError, match="at least one pixel"):               # the shape is looked at before the type
        _lib.label_map(torch.zeros(0, dtype=torch.float32), "labels")


def test_image_planes():
    N, C, H, W = 2, 3, 3, 4
    t = torch.arange(N * C * H * W, dtype=torch.float32).reshape(N, C, H, W)
    got, stride = _lib.image_planes(t[:, 1])                                 # a channel slice is read in place
    assert stride == C * H * W and got.data_ptr() == t[:, 1].data_ptr() and torch.equal(got, t[:, 1])
    got, stride = _lib.image_planes(t[:1, 1])                                # N = 1: the stride is never multiplied by anything but 0
    assert stride == H * W and got.data_ptr() == t[0, 1].data_ptr()
    got, stride = _lib.image_planes(t[:, 0].transpose(1, 2))                 # a transposed map is made contiguous
    assert stride == H * W and got.is_contiguous() and tuple(got.shape) == (N, W, H) and torch.equal(got, t[:, 0].transpose(1, 2))
    got, stride = _lib.image_planes(t[:, 0].double())                        # as is any other type
    assert stride == H * W and got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, t[:, 0])
    got, stride = _lib.image_planes(t[:, :, 1])                              # one row of every channel: the rows are not W apart
    assert stride == H * W and got.is_contiguous() and torch.equal(got, t[:, :, 1])
    g = torch.zeros(2, 3, 4, requires_grad=True)
    assert not _lib.image_planes(g)[0].requires_grad


def test_engine_reexports_the_pointer_helpers():
    from camouflage_multimodal_amd import engine
    assert engine._ptr is _lib._ptr and engine._stream_ptr is _lib._stream_ptr
    assert _lib._ptr(None).value is None and _lib._ptr(torch.zeros(1)).value
