"""The ragged entry points on top of the resize kernel (camouflage_multimodal_amd/pipeline.py, rg_finetune.py): mixed-size uint8 images
in, native-size maps and metrics out, fine-tuning from crops and flips, a directory of files.  Small model (hidden 32, 2 heads),
working size 64 x 64, 30 superpixels.  The resize is exact, so images that already have the working size must give byte for byte
what the fixed-size entry points give, and every native-size map must equal the restatement (tests/resize_ref.py) of the
working-size map.

Two things were measured on the device while writing this file, and both shape it.  (1) torch's ``uint8.float() / 255`` ON THE
DEVICE is not the correctly rounded quotient (it differs from the host's IEEE division in the last bit for 126 of the 256 byte
values); the resize gives the correctly rounded p / 255, as the host does, so the fixed-size inputs are divided on the host.
(2) The fixed-size detector does not repeat ITSELF bit for bit: ``camo_rg_build_csr`` leaves a row's edges in no particular order
and the attention sums follow that order (node probabilities of two calls on the same tensor differed by 6e-8).  That is not the
resize's business, so ``fixed_row_order`` puts every CSR row into one order before the byte comparisons.
"""
import numpy as np
import pytest
import torch

import resize_ref as RR
import slic_ref as SR

SIZE = (64, 64)
NSEG = 30
MIXED = ((48, 80), (96, 64), (64, 64), (96, 64))       # two of equal size: they share a metrics call


@pytest.fixture
def fixed_row_order(monkeypatch):
    """``build_target_csr_device`` with every row's edges after the leading self-loop sorted by source (region graphs have no
    parallel edges): the GNN's sums then depend on the graph alone."""
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
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).cuda().eval()
    for bn in (m.bn1, m.bn2, m.bn3, m.bn4):
        bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    return m


def _scene(shapes, seed=0):
    """uint8 images [H, W, 3] and masks [H, W] (a disc each, bytes 0 / 255; the second mask stays empty)."""
    images, masks = [], []
    for i, (H, W) in enumerate(shapes):
        images.append(np.rint(SR.noise_image(H, W, seed + i) * 255).astype(np.uint8))
        yy, xx = np.mgrid[:H, :W]
        m = np.zeros((H, W), np.uint8)
        if i != 1:
            m[(yy - H * 0.4) ** 2 + (xx - W * 0.55) ** 2 < (min(H, W) * 0.3) ** 2] = 255
        masks.append(m)
    return images, masks


def _same_graphs(a, b):
    return torch.equal(a.x, b.x) and torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_attr, b.edge_attr) \
        and a.node_offsets == b.node_offsets and a.edge_offsets == b.edge_offsets


def _rows(csr):
    """A CSR whose rows are in no particular order after the self-loop, as sorted (row, col, weight bits) triples."""
    rowptr, col, w = (t.cpu().numpy() for t in csr)
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    bits = w.view(np.uint32)
    order = np.lexsort((bits, col, row))
    return rowptr, row[order], col[order], bits[order]


@pytest.mark.gpu
def test_already_sized_images_are_the_fixed_size_path(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage_batch, detect_camouflage_ragged
    m = _model()
    images, masks = _scene([SIZE] * 3, seed=40)
    gt = torch.from_numpy(np.stack(masks)).cuda()
    got = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, cod_metrics=True)
    want = detect_camouflage_batch(m, (torch.from_numpy(np.stack(images)).float() / 255).cuda(), gt, n_segments=NSEG, cod_metrics=True)
    assert set(want) <= set(got) and set(got) - set(want) == {"prob_maps_native", "mask_native"}
    for k in ("prob_maps", "mask", "node_probs", "segments", "region_map"):
        assert torch.equal(got[k], want[k]), k
    assert _same_graphs(got["graphs"], want["graphs"])
    assert got["metrics"] == want["metrics"] and got["cod_metrics"] == want["cod_metrics"]
    for i in range(3):
        assert torch.equal(got["prob_maps_native"][i], got["prob_maps"][i, 0]) and torch.equal(got["mask_native"][i], got["mask"][i])


@pytest.mark.gpu
def test_mixed_sizes_native_maps_and_metrics(fixed_row_order):
    from camouflage_multimodal_amd import (detect_camouflage_batch, detect_camouflage_ragged, resize_batch, seg_measures, segmentation_counts,
                                           segmentation_metrics)
    m = _model()
    images, masks = _scene(MIXED, seed=50)
    out = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=0.45, cod_metrics=True)
    assert tuple(out["prob_maps"].shape) == (4, 3) + SIZE and len(out["prob_maps_native"]) == len(out["mask_native"]) == 4
    small = out["prob_maps"][:, 0].cpu().numpy()
    for i, (shape, native) in enumerate(zip(MIXED, out["prob_maps_native"])):
        assert tuple(native.shape) == shape and native.dtype == torch.float32
        assert np.array_equal(native.cpu().numpy(), RR.resize(small[i], shape, "bilinear")), i
        assert torch.equal(out["mask_native"][i], native > 0.45)
        gt = torch.from_numpy(masks[i]).cuda()
        assert out["metrics"][i] == segmentation_metrics(segmentation_counts(native, gt, 0.45), *shape)[0], i
        assert out["cod_metrics"][i] == seg_measures.cod_metrics(native.unsqueeze(0), gt.unsqueeze(0))[0], i
    assert "metrics" not in detect_camouflage_ragged(m, images, size=SIZE, n_segments=NSEG)

    # the reference's way: the masks resized down (nearest), the score taken at the working size
    low = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=0.45, cod_metrics=True, evaluate_at="resized")
    gt_small = torch.from_numpy(np.stack([RR.resize(g, SIZE, "nearest", out="u8") for g in masks])).cuda()
    want = detect_camouflage_batch(m, resize_batch(images, SIZE), gt_small, n_segments=NSEG, threshold=0.45, cod_metrics=True)
    assert torch.equal(low["prob_maps"], want["prob_maps"]) and torch.equal(low["prob_maps"], out["prob_maps"])
    assert low["metrics"] == want["metrics"] and low["cod_metrics"] == want["cod_metrics"]
    assert [tuple(p.shape) for p in low["prob_maps_native"]] == list(MIXED)


def _same_batches(a, b):
    assert _same_graphs(a.graphs, b.graphs)
    for k in ("segments", "region_map", "mask_target", "instance_target", "edge_target", "counts"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for k in ("csr", "reversed_csr"):
        for u, v in zip(_rows(getattr(a, k)), _rows(getattr(b, k))):
            assert np.array_equal(u, v), k


@pytest.mark.gpu
def test_prepare_finetune_batch_ragged_is_the_fixed_size_path():
    from camouflage_multimodal_amd import prepare_finetune_batch, prepare_finetune_batch_ragged
    images, masks = _scene([SIZE] * 3, seed=60)
    edges = [np.where(np.random.RandomState(i).uniform(size=SIZE) < 0.05, 255, 0).astype(np.uint8) for i in range(3)]
    img = (torch.from_numpy(np.stack(images)).float() / 255).cuda()
    gt, ed = torch.from_numpy(np.stack(masks)).cuda(), torch.from_numpy(np.stack(edges)).cuda()
    got = prepare_finetune_batch_ragged(images, masks, edge_masks=edges, size=SIZE, n_segments=NSEG, band_permille=100)
    _same_batches(got, prepare_finetune_batch(img, gt, edge_masks=ed, n_segments=NSEG, band_permille=100))
    assert {0, 1} <= set(got.mask_target.tolist())
    # column flips on the device against inputs flipped on the host
    flipped = prepare_finetune_batch_ragged(images, masks, edge_masks=edges, size=SIZE, flips=[1, 1, 1], n_segments=NSEG, band_permille=100)
    _same_batches(flipped, prepare_finetune_batch(img.flip(2), gt.flip(2), edge_masks=ed.flip(2), n_segments=NSEG, band_permille=100))
    assert not torch.equal(flipped.segments, got.segments)


@pytest.mark.gpu
def test_step_from_ragged_runs_and_repeats(fixed_row_order):
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN, random_resized_crops
    images, masks = _scene(MIXED, seed=70)
    crops, flips = random_resized_crops(MIXED, seed=1)
    assert any(c != (0, 0, H, W) for c, (H, W) in zip(crops, MIXED))
    params = []
    for _ in range(2):
        torch.manual_seed(11)
        tuner = RegionGraphFineTuner(RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).cuda(), lr=1e-3, seed=5)
        before = tuner.flat_params.clone()
        losses = tuner.step_from_ragged(images, masks, size=SIZE, crops=crops, flips=flips, n_segments=NSEG)
        vals = [float(losses[k]) for k in ("loss", "mask_loss", "instance_loss", "edge_loss")]
        assert len(losses) == 4 and all(np.isfinite(v) for v in vals) and vals[0] > 0
        assert tuner.step_count == 1 and not torch.equal(tuner.flat_params, before)
        params.append(tuner.flat_params.clone())
    assert torch.equal(params[0], params[1])
    tuner.model.eval()
    metrics = tuner.evaluate_ragged(images, masks, size=SIZE, n_segments=NSEG)
    assert len(metrics) == 4 and all(0.0 <= d["iou"] <= 1.0 and d["tp"] + d["fp"] + d["fn"] + d["tn"] == H * W for d, (H, W) in zip(metrics, MIXED))


@pytest.mark.gpu
def test_detect_camouflage_directory(tmp_path, fixed_row_order):
    from PIL import Image
    from camouflage_multimodal_amd import detect_camouflage_directory, detect_camouflage_ragged
    m = _model()
    images, masks = _scene(MIXED, seed=80)
    names = ["b_cat", "a_owl", "d_moth", "c_frog"]
    (tmp_path / "img").mkdir(); (tmp_path / "gt").mkdir()
    for n, im, g in zip(names, images, masks):
        Image.fromarray(im).save(str(tmp_path / "img" / (n + ".png")))
        Image.fromarray(g).save(str(tmp_path / "gt" / (n + ".png")))
    order = sorted(range(4), key=lambda i: names[i])
    got = detect_camouflage_directory(m, str(tmp_path / "img"), str(tmp_path / "gt"), str(tmp_path / "out"), batch_size=3, size=SIZE,
                                      n_segments=NSEG, cod_metrics=True)
    assert got["files"] == sorted(names) and len(got["metrics"]) == len(got["cod_metrics"]) == 4
    for part in (order[:3], order[3:]):                                   # the batches the directory was read in
        want = detect_camouflage_ragged(m, [images[i] for i in part], [masks[i] for i in part], size=SIZE, n_segments=NSEG, cod_metrics=True)
        for k, i in enumerate(part):
            at = sorted(names).index(names[i])
            assert got["metrics"][at] == want["metrics"][k] and got["cod_metrics"][at] == want["cod_metrics"][k], names[i]
            png = np.asarray(Image.open(str(tmp_path / "out" / (names[i] + ".png"))))
            p = want["prob_maps_native"][k].cpu().numpy()
            q = np.rint(np.clip(p, 0, 1).astype(np.float32) * np.float32(255.0)).astype(np.uint8)     # camo_seg_measures.h: fp32 multiply, ties to even
            assert png.dtype == np.uint8 and png.shape == MIXED[i] and np.array_equal(png, q), names[i]
    agg = got["aggregate"]
    assert abs(agg["s_measure"] - sum(c["s_measure"] for c in got["cod_metrics"]) / 4) < 1e-15 and 0.0 <= agg["f_max"] <= 1.0
    assert "f_curve" not in got["cod_metrics"][0] and len(agg["f_curve"]) == 256
