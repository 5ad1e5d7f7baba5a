"""The ``split`` keyword of the detector entry points (camouflage_multimodal_amd/pipeline.py): a fresh
``RegionGraphGNN``, 30 superpixels, built as tests/test_boundary_pipeline.py builds its own.  Off, the keyword changes no key and no
byte; on, the new keys must be ``split.split_instances`` of the call's own instance labels, and the match records and run-length
masks must be those of the split labels.

The detector does not repeat itself bit for bit (``camo_rg_build_csr`` leaves a row's edges in no particular order:
tests/test_resize_pipeline.py), so comparisons between two calls run with every CSR row put into one order."""
import numpy as np
import pytest
import torch

import slic_ref as SR

NSEG = 30
SIZE = (64, 64)
SPLIT = {"ratio": (1, 2), "max_split": 8}                     # (a painted mask of 30 superpixels has shallow necks: a low bar for a core)


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


def _discs(H, W):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), np.uint8)
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
    elif isinstance(a, list) and a and isinstance(a[0], dict) and any(isinstance(v, torch.Tensor) for v in a[0].values()):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same_value(x, y, key)
    elif isinstance(a, dict) and any(isinstance(v, torch.Tensor) for v in a.values()):
        assert list(a) == list(b)
        for k in a:
            _same_value(a[k], b[k], (key, k))
    else:
        assert a == b, key


def _same_dict(a, b):
    assert list(a) == list(b)
    for k in a:
        if k != "graphs":
            _same_value(a[k], b[k], k)


def _split_of(labels, prob, opts, got_records, got_labels, got_counts):
    """The pipeline's split keys of some images against ``split_instances`` / ``split_records`` on their own labels."""
    from camouflage_multimodal_amd import split as S
    o = S.split_options(opts)
    want = S.split_instances(labels, prob, o["ratio"], o["min_core"], o["max_split"], o["max_instances"])
    assert torch.equal(want["labels"], got_labels) and torch.equal(want["counts"], got_counts)
    assert S.split_records(want["table"], want["counts"], *labels.shape[1:]) == got_records
    return want


@pytest.mark.gpu
def test_detect_camouflage_batch_split(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage, detect_camouflage_batch, encode_instances, match_instances
    from camouflage_multimodal_amd.instance_match import ground_truth_labels, match_detected, match_options
    m = _model()
    H, W = 64, 96
    img = torch.from_numpy(np.stack([SR.noise_image(H, W, 20 + i) for i in range(2)])).cuda()
    gt = torch.from_numpy(np.stack([_discs(H, W), _discs(H, W)])).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(n_segments=NSEG, threshold=thr, instances=True, match=True, rle=True, boundary=True)
    base = detect_camouflage_batch(m, img, gt, **kw)
    _same_dict(detect_camouflage_batch(m, img, gt, split=False, **kw), base)
    out = detect_camouflage_batch(m, img, gt, split=SPLIT, **kw)
    assert set(out) - set(base) == {"split_instances", "split_labels", "split_counts"}
    changed = {"instance_match", "instance_match_tables", "boundary_match", "boundary_match_tables", "instance_rles"}
    for k in base:
        if k != "graphs" and k not in changed:
            _same_value(out[k], base[k], k)
    want = _split_of(out["instance_labels"], out["prob_maps"][:, 0], SPLIT, out["split_instances"], out["split_labels"], out["split_counts"])
    assert int(out["split_counts"][:, 1].sum()) >= 1, out["split_counts"].tolist()             # something is split, so the keys below differ
    assert torch.equal(out["split_labels"] > 0, out["instance_labels"] > 0) and not torch.equal(out["split_labels"], out["instance_labels"])
    gt_labels = ground_truth_labels(gt)
    records, tables = match_detected(out["split_labels"], want["table"], gt_labels, match_options(True))
    assert out["instance_match"] == records and out["instance_match"] != base["instance_match"]
    _same_value(out["instance_match_tables"], tables, "instance_match_tables")
    P, G = tables["inter"].shape[1] - 1, tables["inter"].shape[2] - 1
    raw = match_instances(out["split_labels"], gt_labels, want["table"], P, G)
    for k in ("inter", "pred_rows", "match", "gt_match"):
        assert torch.equal(raw[k], out["instance_match_tables"][k]), k
    assert out["instance_rles"] == encode_instances(out["split_labels"]) and out["instance_rles"] != base["instance_rles"]
    assert [len(r) for r in out["instance_rles"]] == out["split_counts"][:, 0].tolist()
    assert [r["n_pred"] for r in out["boundary_match"]] == out["split_counts"][:, 0].tolist()
    one = detect_camouflage(m, img[0], gt[0], n_segments=NSEG, threshold=thr, instances=True, split=SPLIT)
    assert torch.equal(one["split_labels"][0], out["split_labels"][0]) and one["split_instances"] == out["split_instances"][:1]
    same = detect_camouflage_batch(m, img, gt, n_segments=NSEG, threshold=thr, instances=True, split=True)
    _split_of(same["instance_labels"], same["prob_maps"][:, 0], True, same["split_instances"], same["split_labels"], same["split_counts"])


@pytest.mark.gpu
def test_detect_camouflage_ragged_split_at_native_size(fixed_row_order):
    from camouflage_multimodal_amd import detect_camouflage_ragged, encode_instances
    from camouflage_multimodal_amd.instance_match import ground_truth_labels, match_detected, match_options
    m = _model()
    shapes = ((48, 80), (120, 100), (48, 80))                      # two native sizes; the first and the third share a call
    images = [np.rint(SR.noise_image(H, W, 50 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    masks = [_discs(H, W) for H, W in shapes]
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match={"thresholds": [0.5, 0.75]}, rle=True)
    base = detect_camouflage_ragged(m, images, masks, **kw)
    _same_dict(detect_camouflage_ragged(m, images, masks, split=False, **kw), base)
    out = detect_camouflage_ragged(m, images, masks, split=SPLIT, **kw)
    assert set(out) - set(base) == {"split_instances_native", "split_labels_native", "split_counts_native"}
    for k in base:
        if k != "graphs" and k not in ("instance_match", "instance_match_tables", "instance_rles_native"):
            _same_value(out[k], base[k], k)
    assert sum(int(c[1]) for c in out["split_counts_native"]) >= 1, [c.tolist() for c in out["split_counts_native"]]
    for i, (H, W) in enumerate(shapes):
        labels = out["instance_labels_native"][i]
        assert tuple(labels.shape) == (H, W) == tuple(out["split_labels_native"][i].shape)
        want = _split_of(labels[None], out["prob_maps_native"][i][None], SPLIT, [out["split_instances_native"][i]], out["split_labels_native"][i][None],
                         out["split_counts_native"][i][None])
        gt_labels = ground_truth_labels(torch.from_numpy(masks[i]).cuda()[None])
        records, _ = match_detected(want["labels"], want["table"], gt_labels, match_options({"thresholds": [0.5, 0.75]}))
        assert [out["instance_match"][i]] == records
        assert out["instance_rles_native"][i] == encode_instances(want["labels"])[0]


@pytest.mark.gpu
def test_directory_matches_scores_and_writes_the_split_instances(tmp_path, fixed_row_order):
    import json
    from PIL import Image
    from camouflage_multimodal_amd import InstanceAP, detect_camouflage_directory, detect_camouflage_ragged
    from camouflage_multimodal_amd.rle import coco_results
    m = _model()
    shapes = ((48, 80), (96, 64), (48, 80))
    images = [np.rint(SR.noise_image(H, W, 80 + i) * 255).astype(np.uint8) for i, (H, W) in enumerate(shapes)]
    masks = [_discs(H, W) for H, W in shapes]
    names = ["a_owl", "b_cat", "c_frog"]
    (tmp_path / "img").mkdir(); (tmp_path / "gt").mkdir()
    for n, im, g in zip(names, images, masks):
        Image.fromarray(im).save(str(tmp_path / "img" / (n + ".png")))
        Image.fromarray(g).save(str(tmp_path / "gt" / (n + ".png")))
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match=True, split=SPLIT)
    got = detect_camouflage_directory(m, str(tmp_path / "img"), str(tmp_path / "gt"), batch_size=3, results_json=str(tmp_path / "res.json"), **kw)
    want = detect_camouflage_ragged(m, images, masks, rle=True, **kw)
    assert sum(int(c[1]) for c in want["split_counts_native"]) >= 1
    ap = InstanceAP().add(want["instance_match"], [[inst["score"] for inst in r["instances"]] for r in want["split_instances_native"]])
    assert got["instance_match"] == want["instance_match"] and got["instance_ap"] == ap.result()
    assert got["results"] == coco_results(names, want["split_instances_native"], want["instance_rles_native"])
    assert len(got["results"]) == sum(int(c[0]) for c in want["split_counts_native"]) == len(json.load(open(str(tmp_path / "res.json"))))


def test_split_argument_errors_by_name(tmp_path):
    """``ValueError`` before anything touches the device: the model and the images stay on the CPU."""
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage, detect_camouflage_batch, detect_camouflage_directory, detect_camouflage_ragged
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).eval()
    img, gt = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, dtype=torch.uint8)
    ragged, mask = [np.zeros((8, 8, 3), np.uint8)], [np.zeros((8, 8), np.uint8)]
    with pytest.raises(ValueError, match="split needs instances=True"):
        detect_camouflage_batch(m, img, gt, device="cpu", split=True)
    with pytest.raises(ValueError, match="split needs instances=True"):
        detect_camouflage(m, img[0], gt[0], device="cpu", split={"max_split": 2})
    with pytest.raises(ValueError, match="split needs instances=True"):
        detect_camouflage_ragged(m, ragged, mask, device="cpu", split=True)
    with pytest.raises(ValueError, match="split needs instances=True"):
        detect_camouflage_directory(m, str(tmp_path), str(tmp_path), device="cpu", split=True)
    for bad, word in (({"radius": 3}, "split must be"), ("yes", "split must be"), ({"ratio": (7, 7)}, "ratio"), ({"min_core": -1}, "min_core"),
                      ({"max_split": 9}, "max_split"), ({"max_instances": 0}, "max_instances")):
        with pytest.raises(ValueError, match=word):
            detect_camouflage_batch(m, img, gt, device="cpu", instances=True, split=bad)
        with pytest.raises(ValueError, match=word):
            detect_camouflage_ragged(m, ragged, mask, device="cpu", instances=True, split=bad)
    with pytest.raises(TypeError):
        detect_camouflage_batch(m, img, gt, 500, 0.5, "cpu", False, True, 0, False, 8, None, None, False, None, True)      # split is keyword-only
