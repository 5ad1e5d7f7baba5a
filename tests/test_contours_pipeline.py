"""The ``polygons`` keyword of the detector entry points and ``annotations_json`` of the directory call
(camouflage_multimodal_amd/pipeline.py): a fresh ``RegionGraphGNN`` and 30 superpixels, built as
tests/test_boundary_pipeline.py builds its own.  The new key must be the restatement (tests/contours_ref.py) run on the call's own
label maps, every other key must keep its bytes, and the annotations file must read back as the ground truth that matches every
instance to itself.  Comparisons between two calls run with every CSR row put into one order (tests/test_boundary_pipeline.py)."""
import json

import numpy as np
import pytest
import torch

import contours_ref as R
import slic_ref as SR
import test_boundary_pipeline as BP

NSEG, SIZE = BP.NSEG, BP.SIZE
fixed_row_order = BP.fixed_row_order


def _restated(labels, connectivity=8):
    """{id: {"polygons", "holes", "area"}} of one int32 [H, W] label map from the restatement."""
    host = labels.cpu().numpy()
    return {i: {"polygons": o, "holes": h, "area": int((host == i).sum())} for i, (o, h) in sorted(R.polygons(R.trace_image(host, connectivity)[1]).items())}


@pytest.mark.gpu
def test_detect_camouflage_batch_polygons(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage, detect_camouflage_batch
    m = BP._model()
    H, W = 64, 96
    img = torch.from_numpy(np.stack([SR.noise_image(H, W, 20 + i) for i in range(2)])).cuda()
    thr = BP._threshold(detect_camouflage_batch(m, img, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(n_segments=NSEG, threshold=thr, instances=True, rle=True)
    base = detect_camouflage_batch(m, img, **kw)
    off = detect_camouflage_batch(m, img, polygons=False, **kw)
    assert list(off) == list(base)
    for connectivity in (8, 4):
        base = detect_camouflage_batch(m, img, connectivity=connectivity, **kw)
        out = detect_camouflage_batch(m, img, connectivity=connectivity, polygons=True, **kw)
        assert list(out)[:len(base)] == list(base) and set(out) - set(base) == {"instance_polygons"}
        for k in base:
            if k != "graphs":
                BP._same_value(out[k], base[k], k)
        assert out["instance_polygons"] == [_restated(out["instance_labels"][n], connectivity) for n in range(2)]
        for n in range(2):                                           # the ids and areas are the instance table's
            assert {i: e["area"] for i, e in out["instance_polygons"][n].items()} == {r["id"]: r["area"] for r in out["instances"][n]["instances"]}
    assert sum(len(p) for p in out["instance_polygons"]) >= 2
    one = detect_camouflage(m, img[1], n_segments=NSEG, threshold=thr, instances=True, polygons=True)
    assert one["instance_polygons"] == [_restated(one["instance_labels"][0])]


@pytest.mark.gpu
def test_polygons_are_those_of_the_split_labels(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage_batch
    m = BP._model()
    img = torch.from_numpy(np.stack([SR.noise_image(64, 96, 20 + i) for i in range(2)])).cuda()
    thr = BP._threshold(detect_camouflage_batch(m, img, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(n_segments=NSEG, threshold=thr, instances=True, split={"ratio": (9, 10)})
    base = detect_camouflage_batch(m, img, **kw)
    out = detect_camouflage_batch(m, img, polygons=True, **kw)
    assert set(out) - set(base) == {"instance_polygons"}
    for k in base:
        if k != "graphs":
            BP._same_value(out[k], base[k], k)
    assert out["instance_polygons"] == [_restated(out["split_labels"][n]) for n in range(2)]
    assert [sorted(p) for p in out["instance_polygons"]] == [[i["id"] for i in r["instances"]] for r in out["split_instances"]]


@pytest.mark.gpu
def test_detect_camouflage_ragged_polygons_at_native_size(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage_ragged
    m = BP._model()
    shapes = ((48, 80), (120, 100), (48, 80))                        # two native sizes; the first and the third share a call
    images = [np.rint(SR.noise_image(H, W, 50 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    thr = BP._threshold(detect_camouflage_ragged(m, images, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, connectivity=4)
    base = detect_camouflage_ragged(m, images, **kw)
    out = detect_camouflage_ragged(m, images, polygons=True, **kw)
    assert list(out)[:len(base)] == list(base) and set(out) - set(base) == {"instance_polygons_native"}
    for k in base:
        if k != "graphs":
            BP._same_value(out[k], base[k], k)
    assert out["instance_polygons_native"] == [_restated(lab, 4) for lab in out["instance_labels_native"]]
    for (H, W), polys in zip(shapes, out["instance_polygons_native"]):
        flat = [c for e in polys.values() for ring in e["polygons"] for c in ring]
        assert flat and max(flat[0::2]) <= W and max(flat[1::2]) <= H


@pytest.mark.gpu
def test_directory_annotations_read_back_as_their_own_ground_truth(tmp_path, fixed_row_order):
    from PIL import Image
    from camouflage_multimodal_amd import detect_camouflage_directory, detect_camouflage_ragged
    from camouflage_multimodal_amd.polygons import coco_ground_truth, decode_segmentations
    m = BP._model()
    shapes = ((48, 80), (96, 64), (64, 64), (96, 64))
    images = [np.rint(SR.noise_image(H, W, 80 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    names = ["b_cat", "a_owl", "d_moth", "c_frog"]
    (tmp_path / "img").mkdir()
    for n, im in zip(names, images):
        Image.fromarray(im).save(str(tmp_path / "img" / (n + ".png")))
    order = sorted(range(4), key=lambda i: names[i])
    thr = BP._threshold(detect_camouflage_ragged(m, images, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, fill_holes=True, batch_size=3)
    p, q = tmp_path / "annotations.json", tmp_path / "results.json"
    plain = detect_camouflage_directory(m, str(tmp_path / "img"), **kw)
    got = detect_camouflage_directory(m, str(tmp_path / "img"), annotations_json=str(p), results_json=str(q), **kw)
    assert set(got) - set(plain) == {"annotations", "results"} and all(got[k] == plain[k] for k in plain)
    data = json.loads(p.read_text())
    assert data == json.loads(json.dumps(got["annotations"])) and list(data) == ["images", "annotations", "categories"]
    assert data["categories"] == [{"id": 1, "name": "camouflaged"}]
    assert data["images"] == [{"id": names[i], "file_name": names[i], "height": shapes[i][0], "width": shapes[i][1]} for i in order]
    anns = data["annotations"]
    assert [a["id"] for a in anns] == list(range(1, len(anns) + 1)) and len(anns) >= 4 and {a["iscrowd"] for a in anns} == {0}
    assert [(r["image_id"], r["bbox"], r["score"]) for r in got["results"]] == [(a["image_id"], a["bbox"], a["score"]) for a in anns]
    # the file is what coco_ground_truth reads, and painting it gives the instances back: same pixels, same areas
    truth = coco_ground_truth(str(p), sorted(names))
    assert truth["sizes"] == [shapes[i] for i in order] and truth["image_ids"] == {n: n for n in names} and truth["crowd_skipped"] == 0
    native = detect_camouflage_ragged(m, [images[i] for i in order[:3]], size=SIZE, n_segments=NSEG, threshold=thr, instances=True, fill_holes=True)
    for j, i in enumerate(order[:3]):
        mine = [a for a in anns if a["image_id"] == names[i]]
        assert [a["area"] for a in mine] == [r["area"] for r in native["instances_native"][j]["instances"]]
        assert all(a["holes"] == [] and len(a["segmentation"]) == 1 for a in mine)
        if mine:
            painted = decode_segmentations([truth["segmentations"][j]], *shapes[i])[0]
            assert torch.equal(painted, native["instance_labels_native"][j])
    # ... and the same call with the file as ground truth matches every instance to itself
    again = detect_camouflage_directory(m, str(tmp_path / "img"), match={"gt_coco": str(p)}, **kw)
    seen = 0
    for rec in again["instance_match"]:
        assert rec["n_pred"] == rec["n_gt"] and all(pr["best_iou"] == 1.0 and pr["best_gt"] == pr["id"] for pr in rec["predictions"])
        if rec["n_pred"]:
            assert all(t["precision"] == 1.0 and t["recall"] == 1.0 and t["fp"] == t["fn"] == 0 for t in rec["per_threshold"])
            seen += rec["n_pred"]
    assert seen == len(anns) and again["instance_ap"]["AP"] == 1.0 and again["instance_ap"]["AR"] == 1.0
    numbered = detect_camouflage_directory(m, str(tmp_path / "img"), annotations_json=str(p), image_ids={n: 7 + k for k, n in enumerate(names)}, **kw)
    assert [im["id"] for im in numbered["annotations"]["images"]] == [7 + i for i in order]
    assert [a["image_id"] for a in numbered["annotations"]["annotations"]] == [7 + names.index(a["image_id"]) for a in anns]


def test_polygons_argument_errors_by_name(tmp_path):
    """``ValueError`` before anything touches the device: the model and the images stay on the CPU."""
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage, detect_camouflage_batch, detect_camouflage_directory, detect_camouflage_ragged
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).eval()
    img = torch.zeros(1, 16, 16, 3)
    ragged = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match="^polygons needs instances=True"):
        detect_camouflage_batch(m, img, device="cpu", polygons=True)
    with pytest.raises(ValueError, match="^polygons needs instances=True"):
        detect_camouflage(m, img[0], device="cpu", polygons=True)
    with pytest.raises(ValueError, match="^polygons needs instances=True"):
        detect_camouflage_ragged(m, ragged, device="cpu", polygons=True)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="^polygons must be True or False"):
            detect_camouflage_batch(m, img, device="cpu", instances=True, polygons=bad)
        with pytest.raises(ValueError, match="^polygons must be True or False"):
            detect_camouflage_ragged(m, ragged, device="cpu", instances=True, polygons=bad)
    with pytest.raises(ValueError, match="^annotations_json needs instances=True"):
        detect_camouflage_directory(m, str(tmp_path), annotations_json=str(tmp_path / "a.json"), device="cpu")
    with pytest.raises(ValueError, match="^annotations_json must be a path"):
        detect_camouflage_directory(m, str(tmp_path), annotations_json=3, instances=True, device="cpu")
    with pytest.raises(ValueError, match="^image_ids needs results_json or annotations_json"):
        detect_camouflage_directory(m, str(tmp_path), image_ids={"a": 1}, instances=True, device="cpu")
    with pytest.raises(TypeError):
        detect_camouflage_batch(m, img, None, 500, 0.5, "cpu", False, True, 0, False, 8, None, None, False, None, False, True)      # polygons is keyword-only
