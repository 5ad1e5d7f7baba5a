"""The one-launch tail's big weight gradients at B <= 16 (one group of samples).  Needs an MI355X.

tail_fused_kernel leaves the eight products dW += dy^T x of the heads' hidden layers, fusion layers 3 and 0 and the two pooled
FFN layers to extra blocks at the end of the node-level backward's first launch (fused_rows.hip, tail_wg_tile), from copies of
their per-sample operands.  These tests hold those gradients to the separate-launch tail, and the data-parallel tail event to
the point where they are final."""
import numpy as np
import pytest
import torch

from oracle import params as OP
from test_hip_parity import make_model, t2n

pytestmark = pytest.mark.gpu

NRS = [303, 64, 1, 530, 65, 127, 31, 32, 33, 300, 77, 512, 40, 333, 9, 128]
TAIL = ("ffn_rg.3.", "ffn_kg.3.", "fusion_layer.", "mask_head.", "instance_head.", "edge_head.", "score_head.")


def _opt(name, value):
    from camouflage_multimodal_amd import _lib
    _lib.check(_lib.lib().camo_debug_set_option(name.encode(), value), "camo_debug_set_option")


def _batch(eng, B, kg_real):
    nrs = [NRS[i % len(NRS)] for i in range(B)]
    rg = np.concatenate([OP.make_rg(n, 128, seed=40 + i) for i, n in enumerate(nrs)])
    kg = np.stack([kg_real] * B)
    return eng.make_batch(torch.from_numpy(rg).cuda(), nrs, torch.from_numpy(kg).cuda())


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("ncls", [3, 8])
def test_tail_weight_grads_match_separate_launches(B, ncls, kg_real):
    """Every weight and bias gradient of the tail, one-launch tail (weight gradients in the backward's first launch) against the
    ten separate launches, both added to the same non-zero gradients already in the buffer (the training call accumulates)."""
    cfg = OP.full_cfg(dict(num_classes=ncls))
    m = make_model(cfg, 4, "bf16")
    m.train(True)
    eng = m._engine
    batch = _batch(eng, B, kg_real)
    y, e, s = OP.make_labels(B, seed=21)
    g = eng.ensure_flat_grads(attach=True)
    g0 = torch.from_numpy(np.random.default_rng(5).standard_normal(g.numel()).astype(np.float32) * 1e-3).cuda()
    res = []
    try:
        for mode in (-1, 0):
            _opt("tail17", mode)
            ws = eng.workspace(batch, private=True)
            ws.zero_()
            g.copy_(g0)
            _, terms, _ = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, 7, eng._gtab)
            torch.cuda.synchronize()
            res.append((t2n(terms), {k: t2n(p.grad).copy() for k, p in m.named_parameters() if any(t in k for t in TAIL)}))
    finally:
        _opt("tail17", -1)
    (ta, ga), (tb, gb) = res
    assert np.allclose(ta, tb, rtol=2e-6, atol=1e-5)
    assert len(ga) == 24, sorted(ga)
    for k in ga:
        # fp32 on both sides: sums over the samples and the split hidden units in another order (the separate launches: atomics)
        scale = max(float(np.abs(gb[k]).max()), 1e-8)
        assert float(np.abs(ga[k] - gb[k]).max()) <= 3e-4 * scale + 2e-7, (k, float(np.abs(ga[k] - gb[k]).max()), scale)


def test_tail_event_fires_after_the_tail_weight_grads(kg_real):
    """A side stream that waits for the training call's tail event and then copies the tail's run of the flat gradient buffer
    sees the final values: the event is recorded behind the launch that finishes the tail's weight gradients."""
    cfg = OP.full_cfg({})
    m = make_model(cfg, 4, "bf16")
    m.train(True)
    eng = m._engine
    B = 16
    batch = _batch(eng, B, kg_real)
    y, e, s = OP.make_labels(B, seed=22)
    g = eng.ensure_flat_grads(attach=True)
    off = eng.tail_grad_offset()
    ev = torch.cuda.Event()
    ev.record()                                  # (the handle exists once the event has been recorded)
    h = ev.cuda_event
    handle = int(getattr(h, "value", h) or 0)
    assert handle
    side = torch.cuda.Stream()
    snap = torch.empty_like(g[off:])
    for step in range(3):
        ws = eng.workspace(batch, private=True)
        ws.zero_()
        g.zero_()
        torch.cuda.synchronize()
        eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, 11 + step, eng._gtab, tail_event=handle)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            snap.copy_(g[off:])
        torch.cuda.synchronize()
        final = g[off:]
        assert float(final.abs().max()) > 0
        assert torch.equal(snap, final), (step, float((snap - final).abs().max()), int((snap != final).sum()))
