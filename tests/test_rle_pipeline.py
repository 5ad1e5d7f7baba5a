"""The ``rle`` keyword, ``match={"gt_rles": ...}`` and ``results_json`` of the detector entry points (camouflage_multimodal_amd/
pipeline.py): a fresh ``RegionGraphGNN``, 70 x 33 images of bright rectangles on a textured ground, 30
superpixels.  The run-length encodings must decode to the call's own label maps, the RLE ground truth must match as the same ids
given as label maps do, and the keywords left off must change nothing.

The detector does not repeat itself bit for bit (``camo_rg_build_csr`` leaves a row's edges in no particular order:
tests/test_resize_pipeline.py), so comparisons between two calls run with every CSR row put into one order.
"""
import json

import numpy as np
import pytest
import torch

import rle_ref as R
import slic_ref as SR

pytestmark = pytest.mark.gpu
NSEG = 30
SIZE = (64, 64)
BATCH_KEYS = ["prob_maps", "mask", "node_probs", "graphs", "segments", "region_map", "metrics", "instances", "instance_labels", "clean_mask",
              "instance_counts", "clean_metrics"]                      # detect_camouflage_batch with gt_masks and instances=True before this keyword
RAGGED_KEYS = BATCH_KEYS[:6] + ["prob_maps_native", "mask_native", "metrics", "instances_native", "instance_labels_native", "clean_mask_native", "clean_metrics"]


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
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).cuda().eval()
    for bn in (m.bn1, m.bn2, m.bn3, m.bn4):
        bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    return m


def _gt_ids(H, W, empty=False):
    """Two rectangles, ids 1 and 2 (the second overlaps nothing): the ground-truth instances."""
    m = np.zeros((H, W), np.int32)
    if not empty:
        m[H // 8:H // 8 + H // 3, W // 6:W // 6 + W // 2] = 1
        m[H - H // 3:H - 2, W // 2:W - 2] = 2
    return m


def _image(H, W, seed):
    """A textured ground, the two rectangles bright."""
    img = 0.5 * SR.noise_image(H, W, seed)
    img[_gt_ids(H, W) > 0] += 0.45
    return np.clip(img, 0, 1).astype(np.float32)


def _threshold(prob):
    """A threshold between the painted values, so the mask has both classes (a fresh model's probabilities sit close together)."""
    v = torch.unique(prob)
    return float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2) if v.numel() > 1 else 0.5


def _gt_rles(ids):
    from camouflage_multimodal_amd import counts_to_string
    H, W = ids.shape
    return [({"size": [H, W], "counts": counts_to_string(c)}, i) for i, c in R.label_counts(ids).items()]


def _check_rles(rles, labels, records):
    """{id: rle} of one image against its label map [H, W] and its instance records."""
    from camouflage_multimodal_amd import decode_rles, rle_area
    H, W = labels.shape
    assert sorted(rles) == [r["id"] for r in records["instances"]] == list(range(1, records["count"] + 1))
    assert decode_rles([rles], H, W)[0].cpu().numpy().tobytes() == labels.cpu().numpy().tobytes()
    for r in records["instances"]:
        assert rles[r["id"]]["size"] == [H, W] and isinstance(rles[r["id"]]["counts"], str) and rle_area(rles[r["id"]]) == r["area"]


def test_detect_camouflage_batch_rle_and_gt_rles(fixed_row_order):
    from camouflage_multimodal_amd import decode_rles, detect_camouflage, detect_camouflage_batch
    m = _model()
    H, W = 70, 33
    img = torch.from_numpy(np.stack([_image(H, W, 20 + i) for i in range(2)])).cuda()
    ids = np.stack([_gt_ids(H, W), _gt_ids(H, W, empty=True)])
    gt = torch.from_numpy((ids > 0).astype(np.uint8) * 255).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    base = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True)
    off = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True, rle=False, match=None)
    assert list(off) == list(base) == BATCH_KEYS
    for k in ("prob_maps", "mask", "instance_labels", "clean_mask", "instance_counts"):
        assert off[k].cpu().numpy().tobytes() == base[k].cpu().numpy().tobytes(), k

    out = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True, rle=True)
    assert list(out) == BATCH_KEYS + ["instance_rles"]
    for k in ("prob_maps", "mask", "instance_labels", "clean_mask", "instance_counts"):
        assert out[k].cpu().numpy().tobytes() == base[k].cpu().numpy().tobytes(), k
    assert out["instances"] == base["instances"] and sum(r["count"] for r in out["instances"]) >= 1
    assert len(out["instance_rles"]) == 2
    assert decode_rles(out["instance_rles"], H, W).cpu().numpy().tobytes() == out["instance_labels"].cpu().numpy().tobytes()
    for n in range(2):
        _check_rles(out["instance_rles"][n], out["instance_labels"][n], out["instances"][n])
    one = detect_camouflage(m, img[0], gt[0], n_segments=NSEG, threshold=thr, instances=True, rle=True)
    assert list(one) == BATCH_KEYS + ["instance_rles"] and len(one["instance_rles"]) == 1
    _check_rles(one["instance_rles"][0], one["instance_labels"][0], one["instances"][0])

    gt_rles = [_gt_rles(ids[0]), _gt_rles(ids[1])]
    assert len(gt_rles[0]) == 2 and gt_rles[1] == []
    decoded = decode_rles(gt_rles, H, W)
    assert decoded.cpu().numpy().tobytes() == ids.tobytes()
    by_rle = detect_camouflage_batch(m, img, n_segments=NSEG, threshold=thr, instances=True, match={"gt_rles": gt_rles, "thresholds": [0.5, 0.75]})
    by_map = detect_camouflage_batch(m, img, n_segments=NSEG, threshold=thr, instances=True, match={"gt_labels": decoded, "thresholds": [0.5, 0.75]})
    assert list(by_rle) == list(by_map) and by_rle["instance_match"] == by_map["instance_match"] and by_rle["instance_match"][0]["n_gt"] == 2
    for k, v in by_map["instance_match_tables"].items():
        assert torch.equal(by_rle["instance_match_tables"][k], v) if isinstance(v, torch.Tensor) else by_rle["instance_match_tables"][k] == v, k
    with pytest.raises(ValueError, match=r'match\["gt_rles"\] holds 1 lists for 2 images'):
        detect_camouflage_batch(m, img, n_segments=NSEG, threshold=thr, instances=True, match={"gt_rles": gt_rles[:1]})
    with pytest.raises(ValueError, match=r"image 0, annotation 0: size \[33, 70\]"):
        detect_camouflage_batch(m, img, n_segments=NSEG, threshold=thr, instances=True, match={"gt_rles": [[{"size": [33, 70], "counts": [2310]}], []]})


def test_detect_camouflage_ragged_rle_at_native_size(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage_ragged
    m = _model()
    shapes = ((70, 33), (33, 70), (70, 33))                          # two distinct native sizes; the first and the third share a call
    images = [np.rint(_image(H, W, 50 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    ids = [_gt_ids(H, W, empty=i == 1) for i, (H, W) in enumerate(shapes)]
    masks = [(g > 0).astype(np.uint8) * 255 for g in ids]
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    base = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True)
    assert list(base) == RAGGED_KEYS
    assert list(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True, rle=False)) == RAGGED_KEYS
    out = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True, rle=True)
    assert list(out) == RAGGED_KEYS + ["instance_rles_native"] and "instance_rles" not in out and len(out["instance_rles_native"]) == 3
    assert sum(r["count"] for r in out["instances_native"]) >= 1
    for i, (H, W) in enumerate(shapes):
        assert tuple(out["instance_labels_native"][i].shape) == (H, W) and torch.equal(out["instance_labels_native"][i], base["instance_labels_native"][i])
        _check_rles(out["instance_rles_native"][i], out["instance_labels_native"][i], out["instances_native"][i])
    gt_rles = [_gt_rles(g) for g in ids]
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True)
    by_rle = detect_camouflage_ragged(m, images, match={"gt_rles": gt_rles}, **kw)
    by_map = detect_camouflage_ragged(m, images, match={"gt_labels": [torch.from_numpy(g) for g in ids]}, **kw)
    assert by_rle["instance_match"] == by_map["instance_match"] and [r["n_gt"] for r in by_rle["instance_match"]] == [2, 0, 2]
    with pytest.raises(ValueError, match=r"image 2, annotation 0: size \[33, 70\]"):
        detect_camouflage_ragged(m, images, match={"gt_rles": [gt_rles[0], [], [{"size": [33, 70], "counts": [2310]}]]}, **kw)


def test_directory_results_json(tmp_path, fixed_row_order):
    from PIL import Image
    from camouflage_multimodal_amd import decode_rles, detect_camouflage_directory, detect_camouflage_ragged
    m = _model()
    shapes = ((70, 33), (33, 70), (70, 33))
    images = [np.rint(_image(H, W, 80 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    names = ["b_cat", "a_owl", "c_moth"]
    (tmp_path / "img").mkdir()
    for n, im in zip(names, images):
        Image.fromarray(im).save(str(tmp_path / "img" / (n + ".png")))
    order = sorted(range(3), key=lambda i: names[i])
    thr = _threshold(detect_camouflage_ragged(m, images, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True)
    path = tmp_path / "results.json"
    plain = detect_camouflage_directory(m, str(tmp_path / "img"), batch_size=2, **kw)
    got = detect_camouflage_directory(m, str(tmp_path / "img"), batch_size=2, results_json=str(path), **kw)
    assert set(got) - set(plain) == {"results"} and got["files"] == plain["files"] == sorted(names)
    loaded = json.load(open(path))
    assert loaded == got["results"] and len(loaded) >= 1
    want = []
    for part in (order[:2], order[2:]):                                   # the batches the directory was read in
        ref = detect_camouflage_ragged(m, [images[i] for i in part], **kw)
        for i, rec, labels in zip(part, ref["instances_native"], ref["instance_labels_native"]):
            want += [(names[i], shapes[i], inst, labels) for inst in rec["instances"]]
    assert len(loaded) == len(want)
    for entry, (name, (H, W), inst, labels) in zip(loaded, want):
        assert set(entry) == {"image_id", "category_id", "segmentation", "score", "bbox"} and entry["image_id"] == name and entry["category_id"] == 1
        x0, y0, x1, y1 = inst["box"]
        assert entry["bbox"] == [x0, y0, x1 - x0 + 1, y1 - y0 + 1] and entry["score"] == inst["score"]
        assert entry["segmentation"]["size"] == [H, W] and isinstance(entry["segmentation"]["counts"], str)
        mask = decode_rles([[entry["segmentation"]]], H, W)[0]
        assert torch.equal(mask == 1, labels == inst["id"])
    ids = {"a_owl": 7, "b_cat": 11, "c_moth": 13}
    numbered = detect_camouflage_directory(m, str(tmp_path / "img"), batch_size=2, results_json=str(path), image_ids=ids, **kw)
    assert [e["image_id"] for e in json.load(open(path))] == [ids[e["image_id"]] for e in loaded] == [e["image_id"] for e in numbered["results"]]
    with pytest.raises(ValueError, match=r"image_ids has no entry for \['c_moth'\]"):
        detect_camouflage_directory(m, str(tmp_path / "img"), results_json=str(path), image_ids={"a_owl": 7, "b_cat": 11}, **kw)
