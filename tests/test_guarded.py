"""The guard harness itself (tests/guarded.py, tests/raw_calls.py), on CPU tensors: a harness that stopped seeing an overrun would turn
every guard assertion of the suite into a no-op.  The "library" here is a Python function that writes through ctypes.memset and
ctypes.memmove at the pointers it is given; every byte it touches belongs to a tensor the harness made."""
import ctypes

import numpy as np
import pytest

from guarded import GUARD, Arrays, guarded
from raw_calls import BUILDERS, Call, execute, same_bytes

SIZES, SKEWS = (1, 255, 256, 257), (0, 4, 8)
OUTS = {"a": ((3, 5), np.int32), "b": ((7,), np.float64)}
WANT = {k: np.arange(1, 1 + int(np.prod(shape))).reshape(shape).astype(dtype) for k, (shape, dtype) in OUTS.items()}


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("nbytes", SIZES)
def test_a_piece_begins_skew_bytes_past_a_boundary_between_whole_guards(nbytes, skew):
    whole, piece = guarded(nbytes, 0xA5, skew, "cpu")
    at = piece.data_ptr() - whole.data_ptr()
    assert piece.data_ptr() % 256 == skew and piece.numel() == nbytes and at >= GUARD and whole.numel() - at - nbytes >= GUARD
    assert bool((whole == 0xA5).all())
    A = Arrays({"a": nbytes}, 0xA5, skew, "cpu")
    assert A.ptr("a") % 256 == skew and A.ptr("a") == A.piece["a"].data_ptr() and A.nbytes("a") == nbytes


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("nbytes", SIZES)
def test_a_byte_written_either_side_of_a_piece_is_seen_and_the_last_byte_inside_is_not(nbytes, skew):
    for at, seen in ((-1, True), (nbytes, True), (nbytes - 1, False), (0, False)):
        A = Arrays({"first": 16, "a": nbytes, "last": ((2,), np.int64)}, 0xFF, skew, "cpu")
        ctypes.memset(A.ptr("a") + at, 0xFE, 1)
        if seen:
            with pytest.raises(AssertionError, match="a byte outside a was written"):
                A.check_guards()
            with pytest.raises(AssertionError, match="a byte outside a was written"):
                A.collect()
        else:
            got = A.collect()
            assert got["a"][at] == 0xFE and (np.delete(got["a"], at) == 0xFF).all() and (got["last"] == -1).all()


def _write(p, skip=None):
    """Every element of WANT to the pointers ``p``, but for element ``skip`` of "a", which is not touched."""
    for k, w in WANT.items():
        stop = w.nbytes if skip is None or k != "a" else 4 * skip
        ctypes.memmove(p[k], w.ctypes.data, stop)
        ctypes.memmove(p[k] + stop + 4, w.ctypes.data + stop + 4, max(w.nbytes - stop - 4, 0))


def _run(invoke, fill=0xFF, ws=0, ins=None, **kw):
    return execute(Call(OUTS, ws, invoke, ins), fill, device="cpu", error_text=lambda: "the fake call failed", **kw)


def test_execute_returns_what_the_call_wrote_with_dtype_and_shape():
    seen = {}

    def invoke(p, w, nb):
        seen.update(p, ws=(w, nb))
        assert bytes((ctypes.c_ubyte * 6).from_address(p["x"])) == bytes(range(6))      # the input was copied in
        _write(p)
        return 0
    got = _run(invoke, 0xA5, ins={"x": np.arange(6, dtype=np.uint8), "none": np.zeros(0, np.float64)}, skew=4)
    same_bytes(got, WANT, "all written")
    assert seen["none"] is None and seen["ws"] == (None, 0) and seen["a"] % 256 == seen["b"] % 256 == 4 and seen["x"] % 256 == 0


@pytest.mark.parametrize("fill", [0xA5, 0xFF])
def test_an_element_the_call_left_alone_comes_back_as_the_fill(fill):
    got = _run(lambda p, w, nb: _write(p, skip=7) or 0, fill)
    flat = got["a"].reshape(-1)
    assert flat[7:8].tobytes() == bytes([fill] * 4) and (np.delete(flat, 7) == np.delete(WANT["a"].reshape(-1), 7)).all()
    same_bytes(got, WANT, "b", ("b",))
    with pytest.raises(AssertionError):
        same_bytes(got, WANT, "a")


def test_a_changed_input_byte_a_write_past_the_workspace_and_a_return_code_are_seen():
    x = np.arange(40, dtype=np.int32)

    def pokes_input(p, w, nb):
        _write(p)
        ctypes.memset(p["x"] + 37, 0x11, 1)
        return 0
    with pytest.raises(AssertionError, match="the input x was written"):
        _run(pokes_input, ins={"x": x})

    def past_its_size(p, w, nb):
        _write(p)
        ctypes.memset(w, 0, nb)
        if nb == 256:
            ctypes.memset(w + nb, 0, 1)
        return 0
    larger = Call(OUTS, 512, past_its_size)
    assert sorted(_run(past_its_size, ws=512)) == ["a", "b"] and sorted(_run(lambda p, w, nb: _write(p) or 0, ws=256, before=(larger,))) == ["a", "b"]
    with pytest.raises(AssertionError, match="past the size the call was given"):
        _run(past_its_size, ws=256, before=(larger,))
    with pytest.raises(AssertionError, match="a byte outside ws was written"):      # (without the larger call the same byte is the guard's)
        _run(past_its_size, ws=256)
    with pytest.raises(AssertionError, match="the fake call failed"):
        _run(lambda p, w, nb: -1)


HEADERS = ("camo_rg_features.h", "camo_rg_batch.h", "camo_canny.h", "camo_slic.h", "camo_rg_targets.h", "camo_seg_measures.h", "camo_instances.h",
           "camo_inst_match.h", "camo_boundary.h", "camo_guided.h", "camo_rle.h", "camo_poly.h")
LEFT_OUT = ("camo_slic_grid", "camo_slic_preprocess", "camo_slic_assign", "camo_guided_apply")      # no workspace, no accumulator: the modules' tests call them once


def test_the_table_has_a_builder_for_every_call_of_the_pipeline_headers():
    from camouflage_multimodal_amd import _lib
    calls = [s for h in HEADERS for s in _lib.symbols(h) if not s.endswith("_workspace_bytes")] + ["camo_seg_counts"]
    assert len(set(calls)) == len(calls) and not set(BUILDERS) & set(LEFT_OUT)
    assert sorted(calls) == sorted(list(BUILDERS) + list(LEFT_OUT)) and len(BUILDERS) == 19
