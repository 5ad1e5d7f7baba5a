"""sumsq_kernel (csrc/misc.hip) on its own, at the sizes where a grid-stride sum of float4s can go wrong: one element, around one
float4, around one block's float4s (1023 / 1024 / 1025), one short of a multiple of everything (262 143), and the model's parameter
count (1 448 710: what the training step runs, 5.53 grid strides of float4s and a 2-float tail).  Each size with the buffer 16-byte
aligned and offset by 4 bytes (the kernel's n4 = 0 branch: all floats singly).

Against the float64 sum of squares at the bound tests/test_hip_optimizer.py uses for this kernel (oracle/f64_refs.adamw_f64's
``sumsq_bound``: 2 x (ceil(n / 65 536) + 16) u relative + one ulp), for the whole sum and for each of the 256 partial slots against
the elements its block owns -- the slots and their order are the contract with the optimizer kernels that add them up (a
restructured load loop, DESIGN.md 6a round 7, has to keep them).
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import f64_cases as FC
from oracle import f64_refs as R
from oracle import params as OP

pytestmark = pytest.mark.gpu

BLOCKS, PAD, CANARY = 256, 64, -4321.5
MODEL_N = sum(int(v.size) for v in OP.make_params(OP.full_cfg(), 0).values())
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 262143, MODEL_N)


def _bound(n, ref):
    return 2.0 * R.sumsq_rel_error(n) * ref + R.ULP * ref + R.TINY


def _slot_of(n, aligned):
    """The partial slot (block) every element's square goes to: float4 i of the aligned body belongs to thread i mod 65 536 of the
    grid, the floats behind the body (or all of an unaligned buffer) likewise one by one."""
    e = np.arange(n)
    n4 = n // 4 if aligned else 0
    body = e < 4 * n4
    return np.where(body, ((e // 4) % (BLOCKS * 256)) // 256, ((e - 4 * n4) % (BLOCKS * 256)) // 256)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-4-bytes"])
@pytest.mark.parametrize("n", SIZES)
def test_sumsq_partials_against_float64(n, offset):
    from camouflage_multimodal_amd import _lib
    assert MODEL_N == 1448710
    L = _lib.lib()
    st = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    slot = _slot_of(n, offset == 0)
    worst = 0.0
    for kind in ("above", "span"):
        g = FC.adamw_grad(n, kind, n % 71 + offset)
        raw = torch.full((n + 2 * PAD + offset,), CANARY, dtype=torch.float32, device="cuda")
        view = raw[PAD + offset:PAD + offset + n]
        view.copy_(torch.from_numpy(g))
        assert view.data_ptr() % 16 == 4 * offset
        ss = torch.full((1 + BLOCKS + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda")
        out = ss[PAD:PAD + 1 + BLOCKS]
        _lib.check(L.camo_grad_sumsq(C_.c_void_p(view.data_ptr()), n, C_.c_void_p(out.data_ptr()), st), "camo_grad_sumsq")
        torch.cuda.synchronize()
        got = ss.cpu().numpy().astype(np.float64)
        assert (got[:PAD + 1] == CANARY).all() and (got[PAD + 1 + BLOCKS:] == CANARY).all(), "sumsq_kernel wrote outside its 256 partial slots"
        assert np.array_equal(raw.cpu().numpy()[PAD + offset:PAD + offset + n], g), "sumsq_kernel changed the gradient"
        part = got[PAD + 1:PAD + 1 + BLOCKS]
        assert np.isfinite(part).all()
        sq = g.astype(np.float64) ** 2
        want_slots = np.bincount(slot, weights=sq, minlength=BLOCKS)
        ratio = np.abs(part - want_slots) / _bound(n, want_slots)
        b = int(np.argmax(ratio))
        assert ratio[b] <= 1.0, f"n {n} offset {offset} g {kind}: slot {b}: got {part[b]!r} want {want_slots[b]!r} = {ratio[b]:.2f} x bound"
        total, want = float(part.sum()), float(sq.sum())
        r_tot = abs(total - want) / _bound(n, want)
        assert r_tot <= 1.0, f"n {n} offset {offset} g {kind}: sum of the partials {total!r} want {want!r} = {r_tot:.2f} x bound"
        worst = max(worst, float(ratio[b]), r_tot)
    print(f"sumsq_kernel n {n} offset {offset}: largest error / bound {worst:.3f}")
