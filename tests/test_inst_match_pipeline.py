"""The ``match`` keyword of the detector entry points (camouflage_multimodal_amd/pipeline.py, rg_finetune.py, DESIGN.md
10l): a fresh ``RegionGraphGNN``, 30 superpixels.  The new keys must be ``match_instances`` / ``instance_match_records`` of the
call's own label maps, and ``match=None`` must change nothing.

The detector does not repeat itself bit for bit (``camo_rg_build_csr`` leaves a row's edges in no particular order:
tests/test_resize_pipeline.py), so comparisons between two calls run with every CSR row put into one order.
"""
import numpy as np
import pytest
import torch

import slic_ref as SR

NSEG = 30
SIZE = (64, 64)
NAMES = ("inter", "pred_rows", "gt_area", "match", "gt_match", "counts")


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


def _discs(H, W, empty=False):
    """Two discs, bytes 0 / 255: two ground-truth instances."""
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), np.uint8)
    if not empty:
        m[(yy - H * 0.3) ** 2 + (xx - W * 0.3) ** 2 < (min(H, W) * 0.2) ** 2] = 255
        m[(yy - H * 0.7) ** 2 + (xx - W * 0.75) ** 2 < (min(H, W) * 0.15) ** 2] = 255
    return m


def _threshold(prob):
    """A threshold between the painted values, so the mask has both classes (a fresh model's probabilities sit close together)."""
    v = torch.unique(prob)
    return float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2) if v.numel() > 1 else 0.5


def _same_tables(a, b):
    assert a["thresholds"] == b["thresholds"]
    for k in NAMES:
        assert a[k].dtype == torch.int32 and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_detect_camouflage_batch_match(fixed_row_order):
    from fractions import Fraction
    from camouflage_multimodal_amd import detect_camouflage, detect_camouflage_batch, detect_instances, instance_match_records, match_instances
    from camouflage_multimodal_amd.instance_match import COCO, ground_truth_labels
    m = _model()
    H, W = 64, 96
    img = torch.from_numpy(np.stack([SR.noise_image(H, W, 20 + i) for i in range(2)])).cuda()
    gt = torch.from_numpy(np.stack([_discs(H, W), _discs(H, W, empty=True)])).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    base = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True)
    off = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True, match=None)
    assert list(off) == list(base)
    for k in ("prob_maps", "mask", "instance_labels", "clean_mask", "instance_counts", "segments", "node_probs"):
        assert off[k].cpu().numpy().tobytes() == base[k].cpu().numpy().tobytes(), k
    assert off["metrics"] == base["metrics"] and off["instances"] == base["instances"] and off["clean_metrics"] == base["clean_metrics"]

    out = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True, match=True)
    assert list(out)[:len(base)] == list(base) and set(out) - set(base) == {"instance_match", "instance_match_tables"}
    for k in ("prob_maps", "mask", "instance_labels", "clean_mask", "instance_counts"):
        assert out[k].cpu().numpy().tobytes() == base[k].cpu().numpy().tobytes(), k
    assert out["metrics"] == base["metrics"] and out["instances"] == base["instances"]
    found = detect_instances(out["prob_maps"][:, 0], thr)
    assert torch.equal(found["labels"], out["instance_labels"])
    gt_labels = ground_truth_labels(gt)
    assert gt_labels.dtype == torch.int32 and gt_labels.amax(dim=(1, 2)).tolist() == [2, 0]
    direct = match_instances(out["instance_labels"], gt_labels, found["table"], max_gt=64)
    _same_tables(out["instance_match_tables"], direct)
    assert out["instance_match"] == instance_match_records(direct) and out["instance_match_tables"]["thresholds"] == COCO
    rec = out["instance_match"]
    assert len(rec) == 2 and rec[0]["n_gt"] == 2 and rec[1]["n_gt"] == 0 and rec[0]["n_pred"] == out["instances"][0]["count"] >= 1
    assert all(t["tp"] + t["fn"] == 2 and t["tp"] + t["fp"] == rec[0]["n_pred"] for t in rec[0]["per_threshold"]) and rec[0]["pq"] is not None

    # the caller's own ground-truth ids, five of them with a table for three: the second call holds them all
    own = torch.zeros(2, H, W, dtype=torch.int32)
    for k in range(5):
        own[0, 10 * k:10 * k + 8, 5:60] = k + 1
    opt = detect_camouflage_batch(m, img, n_segments=NSEG, threshold=thr, instances=True, match={"thresholds": [0.5, (3, 4)], "gt_labels": own, "max_gt": 3})
    tables = opt["instance_match_tables"]
    assert tables["inter"].shape[2] == 6 and tables["match"].shape[1] == 2 and tables["thresholds"] == (Fraction(1, 2), Fraction(3, 4))
    assert opt["instance_match"][0]["n_gt"] == 5 and not opt["instance_match"][0]["truncated_gt"] and "metrics" not in opt
    _same_tables(tables, match_instances(opt["instance_labels"], own.cuda(), detect_instances(opt["prob_maps"][:, 0], thr)["table"], max_gt=5,
                                         thresholds=[0.5, (3, 4)]))
    one = detect_camouflage(m, img[0], gt[0], n_segments=NSEG, threshold=thr, instances=True, match=True)
    assert len(one["instance_match"]) == 1 and one["instance_match"][0]["n_gt"] == 2


@pytest.mark.gpu
def test_detect_camouflage_ragged_match_at_native_size():
    from camouflage_multimodal_amd import detect_camouflage_ragged, detect_instances, instance_match_records, match_instances
    from camouflage_multimodal_amd.instance_match import ground_truth_labels
    m = _model()
    shapes = ((48, 80), (96, 64), (48, 80))                        # two distinct native sizes; the first and the third share a call
    images = [np.rint(SR.noise_image(H, W, 50 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    masks = [_discs(H, W, empty=i == 1) for i, (H, W) in enumerate(shapes)]
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    base = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True)
    out = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match={"thresholds": [0.5, 0.75]})
    assert list(out)[:len(base)] == list(base) and set(out) - set(base) == {"instance_match", "instance_match_tables"}
    assert len(out["instance_match"]) == len(out["instance_match_tables"]) == 3
    for i, (H, W) in enumerate(shapes):
        labels = out["instance_labels_native"][i]
        assert tuple(labels.shape) == (H, W)
        found = detect_instances(out["prob_maps_native"][i], thr)
        gt_labels = ground_truth_labels(torch.from_numpy(masks[i]).cuda()[None])
        direct = match_instances(labels, gt_labels, found["table"], max_gt=64, thresholds=[0.5, 0.75])
        tables = out["instance_match_tables"][i]
        for k in NAMES:
            assert torch.equal(tables[k], direct[k][0]), (i, k)
        assert int(tables["inter"].sum()) == H * W                   # every native pixel is in one cell: the match is taken at native size
        assert out["instance_match"][i] == instance_match_records(direct)[0]
        assert out["instance_match"][i]["n_gt"] == (0 if i == 1 else 2)
    off = detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match=None)
    assert list(off) == list(base)


@pytest.mark.gpu
def test_directory_instance_ap_and_evaluate(tmp_path, fixed_row_order):
    from PIL import Image
    from camouflage_multimodal_amd import InstanceAP, RegionGraphFineTuner, detect_camouflage_directory, detect_camouflage_ragged
    m = _model()
    shapes = ((48, 80), (96, 64), (64, 64), (96, 64))
    images = [np.rint(SR.noise_image(H, W, 80 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    masks = [_discs(H, W, empty=i == 1) for i, (H, W) in enumerate(shapes)]
    names = ["b_cat", "a_owl", "d_moth", "c_frog"]
    (tmp_path / "img").mkdir(); (tmp_path / "gt").mkdir()
    for n, im, g in zip(names, images, masks):
        Image.fromarray(im).save(str(tmp_path / "img" / (n + ".png")))
        Image.fromarray(g).save(str(tmp_path / "gt" / (n + ".png")))
    order = sorted(range(4), key=lambda i: names[i])
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True)
    got = detect_camouflage_directory(m, str(tmp_path / "img"), str(tmp_path / "gt"), batch_size=3, match=True, **kw)
    plain = detect_camouflage_directory(m, str(tmp_path / "img"), str(tmp_path / "gt"), batch_size=3, **kw)
    assert set(got) - set(plain) == {"instance_match", "instance_ap"} and got["metrics"] == plain["metrics"]
    ap, records = InstanceAP(), []
    for part in (order[:3], order[3:]):                                   # the batches the directory was read in
        want = detect_camouflage_ragged(m, [images[i] for i in part], [masks[i] for i in part], match=True, **kw)
        ap.add(want["instance_match"], [[inst["score"] for inst in r["instances"]] for r in want["instances_native"]])
        records += want["instance_match"]
    assert got["instance_match"] == records and got["instance_ap"] == ap.result()
    res = got["instance_ap"]
    assert res["n_gt"] == 6 and res["n_pred"] >= 1 and 0.0 <= res["AP"] <= 1.0 and 0.0 <= res["AP50"] <= 1.0 and 0.0 <= res["AR"] <= 1.0 and len(res["per_threshold"]) == 10

    tuner = RegionGraphFineTuner(m, lr=1e-3, seed=5)
    m.eval()
    img = torch.from_numpy(np.stack([SR.noise_image(64, 96, 20 + i) for i in range(2)])).cuda()
    gt = torch.from_numpy(np.stack([_discs(64, 96), _discs(64, 96, empty=True)])).cuda()
    assert isinstance(tuner.evaluate(img, gt, n_segments=NSEG, threshold=thr), list)
    ev = tuner.evaluate(img, gt, n_segments=NSEG, threshold=thr, instances=True, match=True)
    assert set(ev) == {"metrics", "instances", "instance_match"} and len(ev["instance_match"]) == len(ev["instances"]) == len(ev["metrics"]) == 2
    assert ev["instance_match"][0]["n_gt"] == 2 and ev["instance_match"][0]["n_pred"] == ev["instances"][0]["count"]
    assert set(tuner.evaluate(img, gt, n_segments=NSEG, threshold=thr, instances=True, cod_metrics=True)) == {"metrics", "instances", "cod_metrics"}
    er = tuner.evaluate_ragged(images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match=True)
    assert set(er) == {"metrics", "instances", "instance_match"} and [r["n_gt"] for r in er["instance_match"]] == [2, 0, 2, 2]
    assert isinstance(tuner.evaluate_ragged(images, masks, size=SIZE, n_segments=NSEG, threshold=thr), list)


def test_match_argument_errors_by_name(tmp_path):
    """``ValueError`` before anything touches the device: the model and the images stay on the CPU."""
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage, detect_camouflage_batch, detect_camouflage_directory, detect_camouflage_ragged
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).eval()
    img, gt = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, dtype=torch.uint8)
    ragged = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match="match needs instances=True"):
        detect_camouflage_batch(m, img, gt, device="cpu", match=True)
    with pytest.raises(ValueError, match="match needs instances=True"):
        detect_camouflage(m, img[0], gt[0], device="cpu", match={"thresholds": [0.5]})
    with pytest.raises(ValueError, match="match needs instances=True"):
        detect_camouflage_ragged(m, ragged, [np.zeros((8, 8), np.uint8)], device="cpu", match=True)
    with pytest.raises(ValueError, match="match needs ground truth"):
        detect_camouflage_batch(m, img, device="cpu", instances=True, match=True)
    with pytest.raises(ValueError, match="match needs ground truth"):
        detect_camouflage_ragged(m, ragged, device="cpu", instances=True, match=True)
    with pytest.raises(ValueError, match="match needs ground truth"):
        detect_camouflage_ragged(m, ragged, [np.zeros((8, 8), np.uint8)], device="cpu", instances=True, evaluate_at="resized", match=True)
    with pytest.raises(ValueError, match="match needs ground truth"):
        detect_camouflage_directory(m, str(tmp_path), device="cpu", instances=True, match=True)
    for bad, word in (({"threshold": [0.5]}, "match must be None, True or a dict"), ("coco", "match must be None, True or a dict"),
                      ({"thresholds": [0.1234]}, "thresholds"), ({"thresholds": []}, "thresholds"), ({"max_gt": 0}, "max_gt"), ({"max_gt": 1025}, "max_gt")):
        with pytest.raises(ValueError, match=word):
            detect_camouflage_batch(m, img, gt, device="cpu", instances=True, match=bad)
    with pytest.raises(TypeError):
        detect_camouflage_batch(m, img, gt, 500, 0.5, "cpu", False, True, 0, False, 8, None, True)      # match is keyword-only
