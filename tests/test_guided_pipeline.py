"""The ``refine`` keyword of the detector entry points (camouflage_multimodal_amd/pipeline.py): a fresh
``RegionGraphGNN``, three 64 x 96 images, 30 superpixels.  The new keys must be ``guided_filter`` / ``guided_upsample`` of the call's
own maps byte for byte, the refined metrics the counts of the call's own refined map, and ``refine=None`` must change nothing.
Nothing here is compared across a threshold against a reference: the kernels are held to tests/guided_ref.py in tests/test_guided.py.

The detector does not repeat itself bit for bit (``camo_rg_build_csr`` leaves a row's edges in no particular order:
tests/test_resize_pipeline.py), so the comparison between two calls runs with every CSR row put into one order.
"""
import numpy as np
import pytest
import torch

import slic_ref as SR

pytestmark = pytest.mark.gpu
NSEG = 30
PARENT_KEYS = ["prob_maps", "mask", "node_probs", "graphs", "segments", "region_map"]


@pytest.fixture
def fixed_row_order(monkeypatch):
    """``build_target_csr_device`` with every row's edges after the leading self-loop sorted by source."""
    from camouflage_multimodal_amd import region_graph, rg_finetune
    real = region_graph.build_target_csr_device

    def canonical(num_nodes, edge_index, edge_weight=None):
        rowptr, col, w = real(num_nodes, edge_index, edge_weight)
        rp = rowptr.long()
        row = torch.repeat_interleave(torch.arange(num_nodes, device=col.device), rp[1:] - rp[:-1])
        first = torch.zeros(col.shape[0], dtype=torch.bool, device=col.device)
        first[rp[:-1]] = True
        order = torch.argsort(row * (num_nodes + 1) + torch.where(first, torch.zeros_like(row), col.long() + 1), stable=True)
        return rowptr, col[order].contiguous(), w[order].contiguous()
    monkeypatch.setattr(region_graph, "build_target_csr_device", canonical)
    monkeypatch.setattr(rg_finetune, "build_target_csr_device", canonical)


def _model(seed=3):
    from camouflage_multimodal_amd import RegionGraphGNN
    torch.manual_seed(seed)
    m = RegionGraphGNN().cuda().eval()
    for bn in (m.bn1, m.bn2, m.bn3, m.bn4):
        bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    return m


def _disc(H, W, empty=False):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), np.uint8)
    if not empty:
        m[(yy - H * 0.4) ** 2 + (xx - W * 0.55) ** 2 < (min(H, W) * 0.3) ** 2] = 255
    return m


def _threshold(prob):
    """A threshold between the painted values, so the mask has both classes (a fresh model's probabilities sit close together)."""
    v = torch.unique(prob)
    return float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2) if v.numel() > 1 else 0.5


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    return a == b


def test_detect_camouflage_batch_refine(fixed_row_order):
    from camouflage_multimodal_amd import (detect_camouflage, detect_camouflage_batch, detect_instances, guided_filter, segmentation_counts,
                                           segmentation_metrics)
    from camouflage_multimodal_amd import refine as RF, seg_measures
    m = _model()
    N, H, W = 3, 64, 96
    img = torch.from_numpy(np.stack([SR.noise_image(H, W, 20 + i) for i in range(N)])).cuda()
    gt = torch.from_numpy(np.stack([_disc(H, W), _disc(H, W, empty=True), _disc(H, W)])).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    plain = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, cod_metrics=True)
    off = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, cod_metrics=True, refine=None)
    assert list(off) == list(plain) == PARENT_KEYS + ["metrics", "cod_metrics"]                    # exactly the parent's keys
    assert list(detect_camouflage_batch(m, img, n_segments=NSEG, threshold=thr)) == PARENT_KEYS

    out = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, cod_metrics=True, refine=True)
    assert list(out) == list(plain) + ["prob_refined", "mask_refined", "refine_coefficients", "refined_metrics", "refined_cod_metrics"]
    for k in plain:
        if k != "graphs":
            assert _same(out[k], plain[k]), k                                                     # every existing key keeps its bytes
    q, coef = guided_filter(img, out["prob_maps"][:, 0], 8, 1e-4, True, True)
    assert _same(out["prob_refined"], q) and _same(out["refine_coefficients"], coef)
    assert tuple(q.shape) == (N, H, W) and tuple(coef.shape) == (N, 4, H, W)
    assert out["mask_refined"].dtype == torch.bool and torch.equal(out["mask_refined"], out["prob_refined"] > thr)
    assert float(q.min()) >= 0.0 and float(q.max()) <= 1.0
    assert not torch.equal(out["prob_refined"], out["prob_maps"][:, 0])
    assert out["refined_metrics"] == segmentation_metrics(segmentation_counts(out["prob_refined"], gt, thr), H, W)
    assert out["refined_cod_metrics"] == seg_measures.cod_metrics(out["prob_refined"], gt)
    assert out["metrics"] == plain["metrics"] and out["cod_metrics"] == plain["cod_metrics"]
    found = detect_instances(out["prob_refined"], thr)                                              # one call away, no new plumbing
    assert len(found["instances"]) == N

    grey = detect_camouflage_batch(m, img, n_segments=NSEG, threshold=thr, refine=dict(guide="gray", radius=4, eps=1e-3))
    assert list(grey) == PARENT_KEYS + ["prob_refined", "mask_refined", "refine_coefficients"]
    luma = 0.2989 * img[..., 0] + 0.5870 * img[..., 1] + 0.1140 * img[..., 2]
    assert torch.equal(luma, RF.luma(img)) and luma.dtype == torch.float32
    q1, c1 = guided_filter(luma, grey["prob_maps"][:, 0], 4, 1e-3, True, True)
    assert _same(grey["prob_refined"], q1) and _same(grey["refine_coefficients"], c1) and tuple(c1.shape) == (N, 2, H, W)

    both = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True, refine=dict(radius=16))
    assert list(both)[-4:] == ["prob_refined", "mask_refined", "refine_coefficients", "refined_metrics"] and "clean_metrics" in both
    one = detect_camouflage(m, img[2], gt[2], n_segments=NSEG, threshold=thr, refine=True)
    assert _same(one["prob_refined"], guided_filter(img[2:3], one["prob_maps"][:, 0], 8, 1e-4, True)) and len(one["refined_metrics"]) == 1
    for bad in ("on", dict(radius=0), dict(eps=0.0), dict(guide="lab")):
        with pytest.raises(ValueError):
            detect_camouflage_batch(m, img, n_segments=NSEG, refine=bad)


def test_detect_camouflage_ragged_refine_at_native_size(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage_ragged, guided_filter, guided_upsample, segmentation_counts, segmentation_metrics
    m = _model()
    shapes = ((48, 80), (96, 64), (70, 45))                          # three images of different sizes
    images = [np.rint(SR.noise_image(H, W, 50 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    masks = [_disc(H, W, empty=i == 1) for i, (H, W) in enumerate(shapes)]
    base = detect_camouflage_ragged(m, images, masks, size=(64, 64), n_segments=NSEG)
    thr = _threshold(base["prob_maps"][:, 0])
    base = detect_camouflage_ragged(m, images, masks, size=(64, 64), n_segments=NSEG, threshold=thr, cod_metrics=True)
    off = detect_camouflage_ragged(m, images, masks, size=(64, 64), n_segments=NSEG, threshold=thr, cod_metrics=True, refine=None)
    assert list(off) == list(base)
    out = detect_camouflage_ragged(m, images, masks, size=(64, 64), n_segments=NSEG, threshold=thr, cod_metrics=True, refine=True)
    assert set(out) - set(base) == {"prob_refined", "mask_refined", "refine_coefficients", "prob_maps_native_refined", "mask_native_refined",
                                   "refined_metrics", "refined_cod_metrics"}
    for k in base:
        if k == "graphs":
            continue
        if isinstance(base[k], list) and base[k] and isinstance(base[k][0], torch.Tensor):
            assert len(out[k]) == len(base[k]) and all(_same(a, b) for a, b in zip(out[k], base[k])), k      # "prob_maps_native" is unchanged
        else:
            assert _same(out[k], base[k]), k
    views, _ = guided_upsample(out["refine_coefficients"], images)
    for i, (H, W) in enumerate(shapes):
        r = out["prob_maps_native_refined"][i]
        assert tuple(r.shape) == (H, W) and r.dtype == torch.float32 and _same(r, views[i])
        assert torch.equal(out["mask_native_refined"][i], r > thr)
        g = torch.from_numpy(masks[i]).cuda()
        assert out["refined_metrics"][i] == segmentation_metrics(segmentation_counts(r, g, thr), H, W)[0]
        assert float(r.min()) >= 0.0 and float(r.max()) <= 1.0
    assert len(out["refined_cod_metrics"]) == 3
    from camouflage_multimodal_amd import resize_batch
    small = resize_batch(images, (64, 64), "bilinear")
    q, coef = guided_filter(small, out["prob_maps"][:, 0], 8, 1e-4, True, True)                    # the filter ran at the working size
    assert _same(out["refine_coefficients"], coef) and _same(out["prob_refined"], q)
    no_gt = detect_camouflage_ragged(m, images, size=(64, 64), n_segments=NSEG, threshold=thr, refine=dict(radius=4))
    assert "refined_metrics" not in no_gt and len(no_gt["prob_maps_native_refined"]) == 3
    with pytest.raises(ValueError):
        detect_camouflage_ragged(m, images, size=(64, 64), n_segments=NSEG, refine=dict(guide="gray"))
