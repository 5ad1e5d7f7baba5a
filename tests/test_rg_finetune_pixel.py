"""The fine-tuner with the structure loss on the painted mask (camouflage_multimodal_amd/rg_finetune.py, include/camo_rg_pixel_loss.h,
DESIGN.md 9e).

The tuner adds no arithmetic of its own: with ``pixel_loss > 0`` a step is camo_rg_loss_backward_pixel (tests/test_rg_pixel_loss.py)
into the flat gradient buffer and the clip + AdamW pair over the flat buffers.  So: ``pixel_loss=0.0`` leaves the bytes of a tuner built
without the argument; with ``pixel_loss=1.0`` a step's figures are loss_and_gradients_csr(pixel=...)'s bytes on the same parameters;
and the flat parameters after one step follow clip_grad_norm_ + torch.optim.AdamW on the float64 gradients of the PIXEL form within the
bound tests/test_rg_finetune.py holds its steps to,

    e = max|d - d64| / max(max|d64|, 1e-12)  <=  8 e32 + 2e-6,

d the update p1 - p0 and e32 the error of the same step in torch-CPU float32 on the float32 gradients of the node form.  The case is
"batch" of tests/test_rg_train.py with the label maps of tests/test_rg_pixel_loss.py (a disc, a full and an empty ground truth).
"""
import numpy as np
import pytest
import torch

import rg_pixel_loss_ref as PR
import rg_train_ref as TR
from test_rg_finetune import BETAS, EPS, HYPER, LR, MAX_NORM, WD, _batch, _padding
from test_rg_pixel_loss import _loss_case
from test_rg_train import NAMES, _bits, _data, _err, _model

KEYS4 = ("loss", "mask_loss", "instance_loss", "edge_loss")
KEYS7 = KEYS4 + ("pixel_loss", "wbce", "wiou")


def _pixel_batch(c, d):
    """tests/test_rg_finetune.py's batch with the three pixel fields, the weights made by the device."""
    from camouflage_multimodal_amd.rg_finetune import pixel_loss_weights
    seg, rmap, off, gt = c["maps"]
    b = _batch(c, d)
    b.pixel_weights = pixel_loss_weights(*[torch.from_numpy(np.array(a)).cuda() for a in (seg, rmap)], [int(v) for v in off],
                                         torch.from_numpy(np.array(gt)).cuda())
    assert np.array_equal(b.pixel_weights.cpu().numpy(), c["node_w"])
    b.node_offsets, b.pixel_radius = torch.from_numpy(np.array(off, np.int32)).cuda(), PR.RADIUS
    return b


def _one_step(c, grads, dtype):
    """clip_grad_norm_ + one torch.optim.AdamW step in `dtype` from the gradients `grads` -> {name: p1 - p0 as float64}, the norm."""
    P = [torch.tensor(np.asarray(c["p"][k]), dtype=dtype, requires_grad=True) for k in NAMES]
    start = [p.detach().clone() for p in P]
    opt = torch.optim.AdamW(P, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    for p, k in zip(P, NAMES):
        p.grad = torch.tensor(np.asarray(grads[k]), dtype=dtype).reshape(p.shape)
    norm = float(torch.nn.utils.clip_grad_norm_(P, MAX_NORM))
    opt.step()
    return {k: (p.detach() - s).double().numpy() for k, p, s in zip(NAMES, P, start)}, norm


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_the_reference_step_clips_and_stays_clear_of_a_relu_flip():
    c = _loss_case("batch", 1.0)
    assert c["margin"] > TR.FLIP_MARGIN
    d64, norm = _one_step(c, c["g64"], torch.float64)
    assert norm > MAX_NORM and all(np.abs(d64[k]).max() > 0 for k in NAMES)
    assert c["l64"][4] > 0 and 0 < c["l64"][5] < 1


def test_batch_fields_default_to_none():
    from camouflage_multimodal_amd import FineTuneBatch
    b = FineTuneBatch(*[None] * 9)
    assert b.pixel_weights is None and b.node_offsets is None and b.pixel_radius is None
    b = FineTuneBatch(*[None] * 9, 1, 2, 3)
    assert (b.pixel_weights, b.node_offsets, b.pixel_radius) == (1, 2, 3)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_zero_weight_is_the_tuner_without_the_argument_after_three_steps():
    from camouflage_multimodal_amd import RegionGraphFineTuner
    c = _loss_case("batch", 1.0)
    d = _data(c)
    plain, zero = RegionGraphFineTuner(_model(c).eval(), **HYPER), RegionGraphFineTuner(_model(c).eval(), pixel_loss=0.0, **HYPER)
    # one CSR pair for both tuners (the device builder leaves a row's edges in no particular order); `plain` steps on a batch that
    # carries the weights, `zero` on one that does not: neither looks
    batch, bare = _pixel_batch(c, d), _batch(c, d)
    bare.csr, bare.reversed_csr = batch.csr, batch.reversed_csr
    for _ in range(3):
        a, b = plain.step(batch), zero.step(bare)
        assert set(a) == set(b) == set(KEYS4)
        for k in KEYS4:
            assert np.array_equal(_bits(a[k].cpu()), _bits(b[k].cpu())), k
    for name, u, v in (("p", plain.flat_params, zero.flat_params), ("g", plain.flat_grads, zero.flat_grads), ("m", plain._m, zero._m),
                       ("v", plain._v, zero._v)):
        assert np.array_equal(_bits(u.cpu()), _bits(v.cpu())), name
    assert plain.step_count == zero.step_count == 3


@pytest.mark.gpu
def test_a_step_is_the_pixel_call_and_follows_the_float64_step():
    from camouflage_multimodal_amd import RegionGraphFineTuner, _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    c = _loss_case("batch", 1.0)
    d64, norm = _one_step(c, c["g64"], torch.float64)
    d32, _ = _one_step(c, c["g32"], torch.float32)
    assert c["margin"] > TR.FLIP_MARGIN and norm > MAX_NORM               # on the CPU reference; the clip is active
    m, d = _model(c).eval(), _data(c)
    start = {k: p.detach().cpu().numpy().astype(np.float64) for k, p in zip(NAMES, m.trainable_parameters())}
    batch = _pixel_batch(c, d)
    pixel = (batch.pixel_weights, batch.node_offsets, batch.pixel_radius, 1.0)
    want, wgrads = _model(c).eval().loss_and_gradients_csr(d.x, batch.csr, batch.reversed_csr, batch.mask_target, batch.instance_target,
                                                           batch.edge_target, pixel=pixel)
    tuner = RegionGraphFineTuner(m, pixel_loss=1.0, **HYPER)
    pad, p0 = _padding(tuner), tuner.flat_params.clone()
    got = tuner.step(batch)
    assert set(got) == set(KEYS7) and all(v.dim() == 0 and v.is_cuda for v in got.values())
    for i, k in enumerate(KEYS4 + ("wbce", "wiou")):
        assert np.array_equal(_bits(got[k].cpu()), _bits(want[i].cpu())), k
    assert float(got["pixel_loss"]) == float(want[4] + want[5])
    # the step is its parts: the call's gradients in a flat buffer, then camo_grad_sumsq and camo_clip_adamw on copies leave the same bytes
    g, mm, vv = torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0)
    ss = torch.zeros(_lib.SUMSQ_FLOATS, dtype=torch.float32, device="cuda")
    for (_, name, o, n, shape), gr in zip(tuner._layout(), wgrads):
        g[o:o + n].copy_(gr.reshape(-1))
    L = _lib.lib()
    _lib.check(L.camo_grad_sumsq(_ptr(g), g.numel(), _ptr(ss), _stream_ptr()), "camo_grad_sumsq")
    _lib.check(L.camo_clip_adamw(_ptr(p0), _ptr(g), _ptr(mm), _ptr(vv), g.numel(), _ptr(ss), MAX_NORM, LR, BETAS[0], BETAS[1], EPS, WD, 1, 0,
                                 _stream_ptr()), "camo_clip_adamw")
    for name, a, b in (("p", tuner.flat_params, p0), ("m", tuner._m, mm), ("v", tuner._v, vv), ("g", tuner.flat_grads, g)):
        assert np.array_equal(_bits(a.cpu()), _bits(b.cpu())), name
    worst = 0.0
    for k, p in zip(NAMES, m.trainable_parameters()):
        upd = p.detach().cpu().numpy().astype(np.float64) - start[k]
        e, e32 = _err(upd, d64[k]), _err(d32[k], d64[k])
        print(f"update {k}: e {e:.3g} e32 {e32:.3g}")
        worst = max(worst, e / e32) if e32 > 0 else worst
        assert e <= 8 * e32 + 2e-6, (k, e, e32)
    print(f"largest e / e32: {worst:.3g}")
    for name, buf in (("p", tuner.flat_params), ("g", tuner.flat_grads), ("m", tuner._m), ("v", tuner._v)):
        assert bool((buf[pad] == 0).all()), name


@pytest.mark.gpu
def test_a_batch_without_the_weights_raises_by_name():
    from camouflage_multimodal_amd import RegionGraphFineTuner
    c = _loss_case("batch", 1.0)
    d = _data(c)
    tuner = RegionGraphFineTuner(_model(c).eval(), pixel_loss=1.0, **HYPER)
    before = tuner.flat_params.clone()
    with pytest.raises(ValueError, match="pixel_weights"):
        tuner.step(_batch(c, d))
    assert tuner.step_count == 0 and torch.equal(tuner.flat_params, before)
    assert set(tuner.step(_pixel_batch(c, d))) == set(KEYS7)


@pytest.mark.gpu
def test_from_images_and_from_ragged_prepare_the_weights():
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN, prepare_finetune_batch, prepare_finetune_batch_ragged
    from test_rg_finetune import _rectangle_images
    from test_resize_pipeline import NSEG, SIZE, _scene
    img, gt = _rectangle_images()
    dimg, dgt = torch.from_numpy(img).cuda(), torch.from_numpy(gt).cuda()
    assert prepare_finetune_batch(dimg, dgt, n_segments=30).pixel_weights is None
    for opt, radius, gain in ((True, 15, 5), ({"radius": 3}, 3, 5), ({"radius": 0, "gain": 16}, 0, 16)):
        batch = prepare_finetune_batch(dimg, dgt, n_segments=30, pixel_loss=opt)
        seg, rmap, off = batch.segments.cpu().numpy(), batch.region_map.cpu().numpy(), batch.graphs.node_offsets
        assert batch.pixel_radius == radius and batch.node_offsets.tolist() == [int(v) for v in off] and batch.node_offsets.is_cuda
        assert np.array_equal(batch.pixel_weights.cpu().numpy(), PR.node_weights(seg, rmap, off, gt, radius, gain))
    assert np.array_equal(batch.pixel_weights.cpu().numpy(), batch.counts.cpu().numpy()[:, :2])      # radius 0: the counts
    torch.manual_seed(3)
    tuner = RegionGraphFineTuner(RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).cuda(), lr=1e-3, loss_weights=(0.0, 1.0, 1.0),
                                 pixel_loss=1.0, pixel_radius=7, pixel_gain=3)
    out = tuner.step_from_images(dimg, dgt, n_segments=30)
    vals = {k: float(v) for k, v in out.items()}
    assert set(out) == set(KEYS7) and all(np.isfinite(v) for v in vals.values()) and vals["wbce"] > 0 and 0 < vals["wiou"] < 1
    images, masks = _scene([SIZE] * 3, seed=60)
    fixed = prepare_finetune_batch((torch.from_numpy(np.stack(images)).float() / 255).cuda(), torch.from_numpy(np.stack(masks)).cuda(),
                                   n_segments=NSEG, pixel_loss={"radius": 7, "gain": 3})
    ragged = prepare_finetune_batch_ragged(images, masks, size=SIZE, n_segments=NSEG, pixel_loss={"radius": 7, "gain": 3})
    assert torch.equal(ragged.pixel_weights, fixed.pixel_weights) and torch.equal(ragged.node_offsets, fixed.node_offsets) and ragged.pixel_radius == 7
    out = tuner.step_from_ragged(images, masks, size=SIZE, n_segments=NSEG)
    assert set(out) == set(KEYS7) and all(np.isfinite(float(v)) for v in out.values()) and tuner.step_count == 2
