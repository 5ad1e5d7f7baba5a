"""The ``boundary`` keyword of the detector entry points (camouflage_multimodal_amd/pipeline.py, rg_finetune.py): a fresh
``RegionGraphGNN``, 30 superpixels, built as tests/test_inst_match_pipeline.py builds its own.  The new keys must be the restatement
(tests/boundary_ref.py) run on the call's own label maps and ground truth, and every other key must keep its bytes.

The detector does not repeat itself bit for bit (``camo_rg_build_csr`` leaves a row's edges in no particular order:
tests/test_resize_pipeline.py), so comparisons between two calls run with every CSR row put into one order."""
import numpy as np
import pytest
import torch

import boundary_ref as B
import slic_ref as SR

NSEG = 30
SIZE = (64, 64)
NAMES = ("inter", "inter_bd", "pred_rows", "gt_area", "match", "gt_match", "counts")


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
    v = torch.unique(prob)
    return float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2) if v.numel() > 1 else 0.5


def _same_value(a, b, key):
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), key
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], torch.Tensor):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same_value(x, y, key)
    elif isinstance(a, (list, tuple, dict, float, int, str)) or a is None:
        if isinstance(a, list) and a and isinstance(a[0], dict) and any(isinstance(v, torch.Tensor) for v in a[0].values()):
            for x, y in zip(a, b):
                for k in x:
                    _same_value(x[k], y[k], (key, k))
        elif isinstance(a, dict) and any(isinstance(v, torch.Tensor) for v in a.values()):
            for k in a:
                _same_value(a[k], b[k], (key, k))
        else:
            assert a == b, key


def _restated(labels, gt_labels, table, d, thresholds, tables, records):
    """One image's "boundary_match_tables" and record against the restatement on its own label map and ground truth."""
    lab, gl = labels.cpu().numpy()[None], gt_labels.cpu().numpy()[None]
    P, G = tables["inter"].shape[-2] - 1, tables["inter"].shape[-1] - 1
    want = B.boundary_match_ref(lab, gl, B.boundary_labels_ref(lab, d), B.boundary_labels_ref(gl, d), P, G, table.cpu().numpy()[None], thresholds)
    for k in NAMES:
        got = tables[k].cpu().numpy()
        assert got.dtype == np.int32 and got.tobytes() == want[k][0].tobytes(), k
    assert (tables["pred_boundary"].cpu().numpy() == B.boundary_labels_ref(lab, d)[0]).all() and tables["distance"] == d == records["distance"]
    assert [t["tp"] for t in records["per_threshold"]] == (want["match"][0] > 0).sum(axis=1).tolist()
    for p in records["predictions"]:
        area, rank, best, i, b_area, ib = (int(v) for v in want["pred_rows"][0, p["id"] - 1])
        assert (p["area"], p["rank"], p["best_gt"], p["boundary_area"]) == (area, rank, best, b_area)
        assert p["matches"] == want["match"][0, :, p["id"] - 1].tolist()
        if best:
            ga, gb = (int(v) for v in want["gt_area"][0, best - 1])
            assert p["best_mask_iou"] == i / (area + ga - i) and p["best_boundary_iou"] == ib / (b_area + gb - ib)
            assert p["best_iou"] == min(p["best_mask_iou"], p["best_boundary_iou"])


def _binary(mask, truth, d):
    """{"boundary_iou", "mask_iou", "distance"} of two bool [H, W] arrays from the restatement."""
    a, b = mask.astype(np.int32), truth.astype(np.int32)
    pa, pb = B.boundary_labels_ref(a, d) > 0, B.boundary_labels_ref(b, d) > 0
    def iou(x, y):
        u = int((x | y).sum())
        return int((x & y).sum()) / u if u else 0.0
    return {"boundary_iou": iou(pa, pb), "mask_iou": iou(a > 0, b > 0), "distance": d}


@pytest.mark.gpu
def test_detect_camouflage_batch_boundary(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage, detect_camouflage_batch, detect_instances
    from camouflage_multimodal_amd.boundary import boundary_distance
    from camouflage_multimodal_amd.instance_match import COCO, ground_truth_labels
    m = _model()
    H, W = 64, 96
    d = boundary_distance(H, W)
    assert d == 2
    img = torch.from_numpy(np.stack([SR.noise_image(H, W, 20 + i) for i in range(2)])).cuda()
    gt = torch.from_numpy(np.stack([_discs(H, W), _discs(H, W, empty=True)])).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(n_segments=NSEG, threshold=thr, instances=True, match=True, refine=True)
    base = detect_camouflage_batch(m, img, gt, **kw)
    off = detect_camouflage_batch(m, img, gt, boundary=None, **kw)
    assert list(off) == list(base)
    out = detect_camouflage_batch(m, img, gt, boundary=True, **kw)
    assert set(out) - set(base) == {"boundary_match", "boundary_match_tables", "boundary_iou", "refined_boundary_iou"}
    for k in base:
        if k != "graphs":
            _same_value(out[k], base[k], k)
    table = detect_instances(out["prob_maps"][:, 0], thr)["table"]
    gt_labels = ground_truth_labels(gt)
    tables = out["boundary_match_tables"]
    assert tables["thresholds"] == COCO and len(out["boundary_match"]) == 2
    for n in range(2):
        _restated(out["instance_labels"][n], gt_labels[n], table[n], d, COCO, {k: (v[n] if isinstance(v, torch.Tensor) else v) for k, v in tables.items()},
                  out["boundary_match"][n])
        truth = gt[n].cpu().numpy() > 127
        assert out["boundary_iou"][n] == _binary(out["mask"][n].cpu().numpy(), truth, d)
        assert out["refined_boundary_iou"][n] == _binary(out["mask_refined"][n].cpu().numpy(), truth, d)
    assert out["boundary_match"][0]["n_gt"] == 2 and out["boundary_match"][0]["n_pred"] == out["instances"][0]["count"] >= 1
    wide = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True, match={"thresholds": [0.5]}, boundary={"distance": 5})
    assert wide["boundary_match_tables"]["distance"] == 5 and wide["boundary_iou"][0]["distance"] == 5 and "refined_boundary_iou" not in wide
    _restated(wide["instance_labels"][0], gt_labels[0], table[0], 5, wide["boundary_match_tables"]["thresholds"],
              {k: (v[0] if isinstance(v, torch.Tensor) else v) for k, v in wide["boundary_match_tables"].items()}, wide["boundary_match"][0])
    one = detect_camouflage(m, img[0], gt[0], n_segments=NSEG, threshold=thr, instances=True, match=True, boundary=True)
    assert len(one["boundary_match"]) == 1 and one["boundary_match"][0]["n_gt"] == 2 and one["boundary_match"][0]["distance"] == d
    assert len(one["boundary_iou"]) == 1 and one["boundary_match_tables"]["pred_rows"].shape[2] == 6


@pytest.mark.gpu
def test_detect_camouflage_ragged_boundary_at_native_size_with_each_sizes_distance():
    from camouflage_multimodal_amd import detect_camouflage_ragged, detect_instances
    from camouflage_multimodal_amd.boundary import boundary_distance
    from camouflage_multimodal_amd.instance_match import ground_truth_labels
    m = _model()
    shapes = ((48, 80), (120, 100), (48, 80))                      # two native sizes, so two distances; the first and the third share a call
    assert [boundary_distance(*s) for s in shapes] == [2, 3, 2]
    images = [np.rint(SR.noise_image(H, W, 50 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    masks = [_discs(H, W, empty=i == 2) for i, (H, W) in enumerate(shapes)]
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match={"thresholds": [0.5, 0.75]})
    base = detect_camouflage_ragged(m, images, masks, **kw)
    out = detect_camouflage_ragged(m, images, masks, boundary=True, **kw)
    assert list(out)[:len(base)] == list(base) and set(out) - set(base) == {"boundary_match", "boundary_match_tables", "boundary_iou"}
    assert len(out["boundary_match"]) == len(out["boundary_match_tables"]) == len(out["boundary_iou"]) == 3
    for i, (H, W) in enumerate(shapes):
        d = boundary_distance(H, W)
        labels = out["instance_labels_native"][i]
        table = detect_instances(out["prob_maps_native"][i], thr)["table"][0]
        gt_labels = ground_truth_labels(torch.from_numpy(masks[i]).cuda()[None])[0]
        _restated(labels, gt_labels, table, d, out["boundary_match_tables"][i]["thresholds"], out["boundary_match_tables"][i], out["boundary_match"][i])
        assert out["boundary_iou"][i] == _binary(out["mask_native"][i].cpu().numpy(), masks[i] > 127, d)


@pytest.mark.gpu
def test_directory_boundary_ap_and_evaluate(tmp_path, fixed_row_order):
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
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match=True)
    got = detect_camouflage_directory(m, str(tmp_path / "img"), str(tmp_path / "gt"), batch_size=3, boundary=True, **kw)
    plain = detect_camouflage_directory(m, str(tmp_path / "img"), str(tmp_path / "gt"), batch_size=3, **kw)
    assert set(got) - set(plain) == {"boundary_match", "boundary_ap", "boundary_iou"}
    for k in plain:
        assert got[k] == plain[k], k
    ap, records, ious = InstanceAP(), [], []
    for part in (order[:3], order[3:]):                                   # the batches the directory was read in
        want = detect_camouflage_ragged(m, [images[i] for i in part], [masks[i] for i in part], boundary=True, **kw)
        ap.add(want["boundary_match"], [[inst["score"] for inst in r["instances"]] for r in want["instances_native"]])
        records += want["boundary_match"]
        ious += want["boundary_iou"]
    assert got["boundary_match"] == records and got["boundary_ap"] == ap.result() and got["boundary_iou"] == ious
    res = got["boundary_ap"]
    assert res["n_gt"] == 6 and res["n_pred"] == plain["instance_ap"]["n_pred"] and len(res["per_threshold"]) == 10

    tuner = RegionGraphFineTuner(m, lr=1e-3, seed=5)
    m.eval()
    img = torch.from_numpy(np.stack([SR.noise_image(64, 96, 20 + i) for i in range(2)])).cuda()
    gt = torch.from_numpy(np.stack([_discs(64, 96), _discs(64, 96, empty=True)])).cuda()
    ev = tuner.evaluate(img, gt, n_segments=NSEG, threshold=thr, instances=True, match=True, boundary=True)
    assert set(ev) == {"metrics", "instances", "instance_match", "boundary_match", "boundary_iou"} and len(ev["boundary_match"]) == 2
    assert ev["boundary_match"][0]["n_gt"] == 2 and ev["boundary_match"][0]["distance"] == 2 and "boundary_area" in ev["boundary_match"][0]["predictions"][0]
    assert set(tuner.evaluate(img, gt, n_segments=NSEG, threshold=thr, instances=True, match=True)) == {"metrics", "instances", "instance_match"}
    er = tuner.evaluate_ragged(images, masks, size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match=True, boundary={"ratio": 0.05})
    assert [r["n_gt"] for r in er["boundary_match"]] == [2, 0, 2, 2] and [r["distance"] for r in er["boundary_match"]] == [5, 6, 5, 6]


def test_boundary_argument_errors_by_name(tmp_path):
    """``ValueError`` before anything touches the device: the model and the images stay on the CPU."""
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage, detect_camouflage_batch, detect_camouflage_directory, detect_camouflage_ragged
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).eval()
    img, gt = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, dtype=torch.uint8)
    ragged, mask = [np.zeros((8, 8, 3), np.uint8)], [np.zeros((8, 8), np.uint8)]
    with pytest.raises(ValueError, match="boundary needs match"):
        detect_camouflage_batch(m, img, gt, device="cpu", instances=True, boundary=True)
    with pytest.raises(ValueError, match="boundary needs match"):
        detect_camouflage(m, img[0], gt[0], device="cpu", boundary={"distance": 3})
    with pytest.raises(ValueError, match="boundary needs match"):
        detect_camouflage_ragged(m, ragged, mask, device="cpu", instances=True, boundary=True)
    with pytest.raises(ValueError, match="boundary needs match"):
        detect_camouflage_directory(m, str(tmp_path), str(tmp_path), device="cpu", instances=True, boundary=True)
    for bad, word in (({"d": 3}, "boundary must be None, True or a dict"), ("yes", "boundary must be None, True or a dict"), ({"distance": 0}, "distance"),
                      ({"distance": 4097}, "distance"), ({"distance": 1.5}, "distance"), ({"ratio": 0}, "ratio"), ({"ratio": 2}, "ratio")):
        with pytest.raises(ValueError, match=word):
            detect_camouflage_batch(m, img, gt, device="cpu", instances=True, match=True, boundary=bad)
        with pytest.raises(ValueError, match=word):
            detect_camouflage_ragged(m, ragged, mask, device="cpu", instances=True, match=True, boundary=bad)
    with pytest.raises(TypeError):
        detect_camouflage_batch(m, img, gt, 500, 0.5, "cpu", False, True, 0, False, 8, None, True, False, True)      # boundary is keyword-only
