"""``match={"gt_segmentations": ...}`` and ``match={"gt_coco": ...}`` of the detector entry points (camouflage_multimodal_amd/
pipeline.py): a fresh ``RegionGraphGNN``, 70 x 33 images of bright rectangles on a textured ground, 30
superpixels, as tests/test_rle_pipeline.py.  Ground truth given as COCO polygons must match as the maps tests/poly_ref.py restates
from the same polygons do, and with the keys absent the calls return the keys they returned before.

The detector does not repeat itself bit for bit (``camo_rg_build_csr`` leaves a row's edges in no particular order:
tests/test_resize_pipeline.py), so comparisons between two calls run with every CSR row put into one order.
"""
import json

import numpy as np
import pytest
import torch

import poly_ref as P
import rle_ref as R
import slic_ref as SR

pytestmark = pytest.mark.gpu
NSEG = 30
SIZE = (64, 64)
BATCH_KEYS = ["prob_maps", "mask", "node_probs", "graphs", "segments", "region_map", "metrics", "instances", "instance_labels", "clean_mask",
              "instance_counts", "clean_metrics"]                      # detect_camouflage_batch with gt_masks and instances=True, no match
RAGGED_KEYS = BATCH_KEYS[:6] + ["prob_maps_native", "mask_native", "metrics", "instances_native", "instance_labels_native", "clean_mask_native", "clean_metrics"]
MATCH_KEYS = ["instance_match", "instance_match_tables"]


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


def _boxes(H, W, empty=False):
    """Two rectangles (x0, y0, x1, y1), ids 1 and 2 in list order; the second overlaps nothing."""
    return [] if empty else [(W // 6, H // 8, W // 6 + W // 2, H // 8 + H // 3), (W // 2, H - H // 3, W - 2, H - 2)]


def _polygons(H, W, empty=False):
    """The rectangles as COCO segmentations: one polygon list per instance (integer corners fill x0 <= x < x1, y0 <= y < y1)."""
    return [[[float(v) for v in (x0, y0, x1, y0, x1, y1, x0, y1)]] for x0, y0, x1, y1 in _boxes(H, W, empty)]


def _gt_ids(H, W, empty=False):
    m = np.zeros((H, W), np.int32)
    for i, (x0, y0, x1, y1) in enumerate(_boxes(H, W, empty)):
        m[y0:y1, x0:x1] = i + 1
    return m


def _restated(H, W, empty=False):
    ids = P.label_map([(polys, i + 1) for i, polys in enumerate(_polygons(H, W, empty))], H, W)
    assert ids.tobytes() == _gt_ids(H, W, empty).tobytes()
    return ids


def _image(H, W, seed):
    img = 0.5 * SR.noise_image(H, W, seed)
    img[_gt_ids(H, W) > 0] += 0.45
    return np.clip(img, 0, 1).astype(np.float32)


def _threshold(prob):
    """A threshold between the painted values, so the mask has both classes (a fresh model's probabilities sit close together)."""
    v = torch.unique(prob)
    return float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2) if v.numel() > 1 else 0.5


def _same_tables(got, want):
    for k, v in want.items():
        assert torch.equal(got[k], v) if isinstance(v, torch.Tensor) else got[k] == v, k


def test_detect_camouflage_batch_gt_segmentations(fixed_row_order):
    from camouflage_multimodal_amd import counts_to_string, detect_camouflage, detect_camouflage_batch
    m = _model()
    H, W = 70, 33
    img = torch.from_numpy(np.stack([_image(H, W, 20 + i) for i in range(2)])).cuda()
    ids = np.stack([_restated(H, W), _restated(H, W, empty=True)])
    gt = torch.from_numpy((ids > 0).astype(np.uint8) * 255).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    base = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True)
    assert list(base) == BATCH_KEYS                                    # with the key absent: the keys of before
    kw = dict(n_segments=NSEG, threshold=thr, instances=True)
    segs = [_polygons(H, W), _polygons(H, W, empty=True)]
    by_poly = detect_camouflage_batch(m, img, match={"gt_segmentations": segs, "thresholds": [0.5, 0.75]}, **kw)
    by_map = detect_camouflage_batch(m, img, match={"gt_labels": torch.from_numpy(ids).cuda(), "thresholds": [0.5, 0.75]}, **kw)
    assert list(by_poly) == list(by_map) == [k for k in BATCH_KEYS if "metrics" not in k] + MATCH_KEYS
    assert by_poly["instance_match"] == by_map["instance_match"] and [r["n_gt"] for r in by_poly["instance_match"]] == [2, 0]
    _same_tables(by_poly["instance_match_tables"], by_map["instance_match_tables"])
    # the second instance as an RLE with an id of its own, the first as a polygon: both kinds in one image
    rle = {"size": [H, W], "counts": counts_to_string(R.mask_counts(ids[0] == 2))}
    mixed = detect_camouflage_batch(m, img, match={"gt_segmentations": [[(rle, 2), (segs[0][0], 1)], []], "thresholds": [0.5, 0.75]}, **kw)
    assert mixed["instance_match"] == by_map["instance_match"]
    one = detect_camouflage(m, img[0], match={"gt_segmentations": segs[:1], "thresholds": [0.5, 0.75]}, **kw)
    assert one["instance_match"] == by_map["instance_match"][:1]
    with pytest.raises(ValueError, match=r'match\["gt_segmentations"\] holds 1 lists for 2 images'):
        detect_camouflage_batch(m, img, match={"gt_segmentations": segs[:1]}, **kw)
    with pytest.raises(ValueError, match="image 1, annotation 0: a polygon with an odd number of coordinates"):
        detect_camouflage_batch(m, img, match={"gt_segmentations": [segs[0], [[[1, 2, 3]]]]}, **kw)


def test_detect_camouflage_ragged_gt_segmentations_at_native_size(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage_ragged
    m = _model()
    shapes = ((70, 33), (33, 70), (70, 33))                          # two distinct native sizes; the first and the third share a call
    images = [np.rint(_image(H, W, 50 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    ids = [_restated(H, W, empty=i == 1) for i, (H, W) in enumerate(shapes)]
    masks = [(g > 0).astype(np.uint8) * 255 for g in ids]
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    assert list(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True)) == RAGGED_KEYS
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True)
    segs = [_polygons(H, W, empty=i == 1) for i, (H, W) in enumerate(shapes)]
    by_poly = detect_camouflage_ragged(m, images, match={"gt_segmentations": segs}, **kw)
    by_map = detect_camouflage_ragged(m, images, match={"gt_labels": [torch.from_numpy(g) for g in ids]}, **kw)
    assert list(by_poly) == list(by_map) == [k for k in RAGGED_KEYS if "metrics" not in k] + MATCH_KEYS
    assert by_poly["instance_match"] == by_map["instance_match"] and [r["n_gt"] for r in by_poly["instance_match"]] == [2, 0, 2]
    for got, want in zip(by_poly["instance_match_tables"], by_map["instance_match_tables"]):
        _same_tables(got, want)
    with pytest.raises(ValueError, match="image 2, annotation 1: an empty polygon"):
        detect_camouflage_ragged(m, images, match={"gt_segmentations": [segs[0], [], [segs[2][0], [[]]]]}, **kw)
    with pytest.raises(ValueError, match=r'match\["gt_segmentations"\] holds 2 lists for 3 images'):
        detect_camouflage_ragged(m, images, match={"gt_segmentations": segs[:2]}, **kw)


def test_directory_gt_coco(tmp_path, fixed_row_order):
    from PIL import Image
    from camouflage_multimodal_amd import counts_to_string, detect_camouflage_directory, detect_camouflage_ragged
    m = _model()
    shapes = ((70, 33), (33, 70), (70, 33), (33, 70))
    images = [np.rint(_image(H, W, 80 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    names = ["b_cat", "a_owl", "c_moth", "d_frog"]
    (tmp_path / "img").mkdir()
    for n, im in zip(names, images):
        Image.fromarray(im).save(str(tmp_path / "img" / (n + ".png")))
    order = sorted(range(4), key=lambda i: names[i])
    coco = {"images": [{"id": 100 + i, "file_name": names[i] + ".png", "height": shapes[i][0], "width": shapes[i][1]} for i in range(4)], "annotations": []}
    for i, (H, W) in enumerate(shapes):
        if i == 1:                                                     # a_owl: its second instance as an RLE, and a crowd that is left out
            polys = _polygons(H, W)
            coco["annotations"] += [{"image_id": 101, "iscrowd": 0, "segmentation": polys[0]},
                                    {"image_id": 101, "iscrowd": 0, "segmentation": {"size": [H, W], "counts": counts_to_string(R.mask_counts(_gt_ids(H, W) == 2))}},
                                    {"image_id": 101, "iscrowd": 1, "segmentation": {"size": [H, W], "counts": [0, H * W]}}]
        else:
            coco["annotations"] += [{"image_id": 100 + i, "iscrowd": 0, "segmentation": p} for p in _polygons(H, W, empty=i == 2)]
    ids = [_restated(H, W, empty=i == 2) for i, (H, W) in enumerate(shapes)]
    thr = _threshold(detect_camouflage_ragged(m, images, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True)
    folder = str(tmp_path / "img")
    plain = detect_camouflage_directory(m, folder, batch_size=3, **kw)
    assert list(plain) == ["files"]                                    # with the key absent: the keys of before
    by_map = detect_camouflage_directory(m, folder, batch_size=3, match={"gt_labels": [torch.from_numpy(ids[i]) for i in order]}, **kw)
    path = tmp_path / "results.json"
    by_coco = detect_camouflage_directory(m, folder, batch_size=3, match={"gt_coco": coco}, results_json=str(path), **kw)
    assert set(by_coco) - set(by_map) == {"results"} and by_coco["files"] == sorted(names)
    assert by_coco["instance_match"] == by_map["instance_match"] and by_coco["instance_ap"] == by_map["instance_ap"]
    assert [r["n_gt"] for r in by_coco["instance_match"]] == [2, 2, 0, 2]
    loaded = json.load(open(path))
    assert loaded == by_coco["results"] and len(loaded) >= 1 and {e["image_id"] for e in loaded} <= {100, 101, 102, 103}
    named = detect_camouflage_directory(m, folder, batch_size=3, results_json=str(path), **kw)["results"]
    assert [e["image_id"] for e in loaded] == [100 + names.index(e["image_id"]) for e in named]
    (tmp_path / "coco.json").write_text(json.dumps(coco))
    from_file = detect_camouflage_directory(m, folder, batch_size=3, match={"gt_coco": str(tmp_path / "coco.json")}, **kw)
    assert from_file["instance_match"] == by_map["instance_match"] and "results" not in from_file
    keep = detect_camouflage_directory(m, folder, batch_size=3, match={"gt_coco": coco}, results_json=str(path), image_ids={n: n.upper() for n in names}, **kw)
    assert {e["image_id"] for e in keep["results"]} <= {n.upper() for n in names}      # the caller's ids win
    wrong = dict(coco, images=[dict(im, height=im["width"], width=im["height"]) if im["id"] == 103 else im for im in coco["images"]])
    with pytest.raises(ValueError, match="d_frog is 33 x 70 and the annotations state 70 x 33"):
        detect_camouflage_directory(m, folder, batch_size=3, match={"gt_coco": wrong}, **kw)
    with pytest.raises(ValueError, match="no image named 'd_frog'"):
        detect_camouflage_directory(m, folder, match={"gt_coco": dict(coco, images=coco["images"][:3])}, **kw)
