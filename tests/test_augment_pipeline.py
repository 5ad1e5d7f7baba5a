"""The augmentation on top of its kernels (camouflage_multimodal_amd/augment.py, rg_finetune.py): ``augment_batch``
against ``resize_batch`` where the two state the same thing, and the ``augment=`` keyword of the ragged fine-tuning entry points.
Small model (hidden 32, 2 heads), working size 64 x 64, 30 superpixels, four images of 40 .. 90 pixels a side.
"""
import numpy as np
import pytest
import torch

import augment_ref as AR
import slic_ref as SR
from test_resize_pipeline import _same_batches, fixed_row_order  # noqa: F401  (the fixture that puts every CSR row into one order)

SIZE = (64, 64)
NSEG = 30
MIXED = ((48, 80), (90, 64), (64, 64), (40, 77))


def _scene(shapes, seed=0):
    """uint8 images [H, W, 3] and masks [H, W] (a disc each, bytes 0 / 255); channel 0 of every image IS its mask."""
    images, masks = [], []
    for i, (H, W) in enumerate(shapes):
        img = np.rint(SR.noise_image(H, W, seed + i) * 255).astype(np.uint8)
        yy, xx = np.mgrid[:H, :W]
        m = np.zeros((H, W), np.uint8)
        m[(yy - H * 0.4) ** 2 + (xx - W * 0.55) ** 2 < (min(H, W) * 0.3) ** 2] = 255
        img[:, :, 0] = m
        images.append(img)
        masks.append(m)
    return images, masks


@pytest.mark.gpu
def test_crops_and_flips_alone_are_resize_batch():
    from camouflage_multimodal_amd import pack_images, random_resized_crops, resize_batch
    from camouflage_multimodal_amd.augment import affine_rows, augment_batch
    images, masks = _scene(MIXED, seed=10)
    packed = pack_images(images)
    crops, flips = random_resized_crops(MIXED, seed=2)
    flips = [(f + i) % 4 for i, f in enumerate(flips)]
    rows = affine_rows(MIXED, SIZE, crops, flips, border="replicate")
    for dtype in (torch.float32, torch.uint8):
        assert torch.equal(augment_batch(packed, SIZE, rows, out_dtype=dtype), resize_batch(packed, SIZE, "bilinear", crops, flips, out_dtype=dtype)), dtype
    assert torch.equal(augment_batch(masks, SIZE, rows, filter="nearest", out_dtype=torch.uint8),
                       resize_batch(masks, SIZE, "nearest", crops, flips, out_dtype=torch.uint8))
    assert torch.equal(augment_batch(packed, SIZE), resize_batch(packed, SIZE))                  # no rows: the whole image, its edge repeated


@pytest.mark.gpu
def test_augment_none_is_the_call_without_the_keyword():
    from camouflage_multimodal_amd import prepare_finetune_batch_ragged, random_resized_crops
    images, masks = _scene(MIXED, seed=20)
    crops, flips = random_resized_crops(MIXED, seed=3)
    for kw in (dict(), dict(crops=crops, flips=flips)):
        a = prepare_finetune_batch_ragged(images, masks, size=SIZE, n_segments=NSEG, band_permille=100, **kw)
        b = prepare_finetune_batch_ragged(images, masks, size=SIZE, n_segments=NSEG, band_permille=100, augment=None, **kw)
        _same_batches(a, b)


@pytest.mark.gpu
def test_masks_turn_with_their_images():
    """Channel 0 of every image is its mask.  The image goes through the maps bilinear and the mask nearest.  The nearest tap is
    the one of the four whose weight in x and in y is at least a half, so its weight is at least a quarter: where the bilinear
    value of the 0 / 255 channel is above 3/4 the nearest byte is 255, below 1/4 it is 0.  That is the whole nearest-against-bilinear
    difference at the contour; any misalignment of a pixel breaks it along the disc's edge."""
    from camouflage_multimodal_amd import prepare_finetune_batch, prepare_finetune_batch_ragged
    from camouflage_multimodal_amd.augment import affine_rows, augment_batch, random_cod_augmentation
    images, masks = _scene(MIXED, seed=30)
    aug = random_cod_augmentation(MIXED, SIZE, seed=4, rotate_p=1.0)
    assert all(a != 0.0 for a in aug["angles"]) and aug["factors"] is not None
    rows = affine_rows(MIXED, SIZE, aug["crops"], aug["flips"], aug["angles"])
    img = augment_batch(images, SIZE, rows)
    m = augment_batch(masks, SIZE, rows, filter="nearest", out_dtype=torch.uint8)
    ch0 = img[..., 0]
    assert set(m.unique().tolist()) == {0, 255}
    assert bool((m[ch0 > 0.75] == 255).all()) and bool((m[ch0 < 0.25] == 0).all())
    assert int((ch0 > 0.75).sum()) > 200 and int((ch0 < 0.25).sum()) > 200 and int(((ch0 > 0.0) & (ch0 < 1.0)).sum()) > 50
    plain = augment_batch(masks, SIZE, affine_rows(MIXED, SIZE, aug["crops"], aug["flips"]), filter="nearest", out_dtype=torch.uint8)
    assert not torch.equal(plain, m)                                       # the turn does something
    for i, (im, r) in enumerate(zip(images, rows)):                       # and both are the restatement's bytes
        assert np.array_equal(m[i].cpu().numpy(), AR.warp(masks[i], SIZE, r[:4], r[4:10], r[10], r[11], "nearest", "u8")), i
        assert np.array_equal(img[i].cpu().numpy(), AR.warp(im, SIZE, r[:4], r[4:10], r[10], r[11], "bilinear", "f32")), i
    # the entry point sends the image and every mask through these very maps, the image with the factors
    got = prepare_finetune_batch_ragged(images, masks, edge_masks=masks, size=SIZE, n_segments=NSEG, band_permille=100, augment=aug)
    want = prepare_finetune_batch(augment_batch(images, SIZE, rows, aug["factors"]), m, edge_masks=m, n_segments=NSEG, band_permille=100)
    _same_batches(got, want)
    assert {0, 1} <= set(got.mask_target.tolist())
    unenhanced = prepare_finetune_batch(img, m, edge_masks=m, n_segments=NSEG, band_permille=100)
    assert not torch.equal(unenhanced.graphs.x, got.graphs.x)             # node features are colour statistics: the factors reach them


@pytest.mark.gpu
def test_step_from_ragged_with_augment_runs_and_repeats(fixed_row_order):
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN
    from camouflage_multimodal_amd.augment import random_cod_augmentation
    images, masks = _scene(MIXED, seed=40)
    params = []
    for _ in range(2):
        aug = random_cod_augmentation(MIXED, SIZE, seed=6, rotate_p=0.5)
        torch.manual_seed(11)
        tuner = RegionGraphFineTuner(RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).cuda(), lr=1e-3, seed=5)
        before = tuner.flat_params.clone()
        losses = tuner.step_from_ragged(images, masks, size=SIZE, n_segments=NSEG, augment=aug)
        vals = [float(losses[k]) for k in ("loss", "mask_loss", "instance_loss", "edge_loss")]
        assert len(losses) == 4 and all(np.isfinite(v) for v in vals) and vals[0] > 0
        assert tuner.step_count == 1 and not torch.equal(tuner.flat_params, before)
        params.append(tuner.flat_params.clone())
    assert torch.equal(params[0], params[1])
    with pytest.raises(ValueError, match="crops and flips"):
        tuner.step_from_ragged(images, masks, size=SIZE, n_segments=NSEG, augment=aug, crops=aug["crops"])
