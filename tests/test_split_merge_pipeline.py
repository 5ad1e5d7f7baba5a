"""``merge`` from ``split.split_instances`` up through the detector entry points and ``RegionGraphFineTuner.evaluate``
(camouflage_multimodal_amd/split.py, pipeline.py, rg_finetune.py).  The model, the images and the row order of the
CSR are those of tests/test_split_pipeline.py; the lobe is tests/test_split_merge.py's.  Everywhere the merged keys must be
``split.merge_parts`` of the unmerged call's own split labels, and without "merge" no key and no byte changes."""
import numpy as np
import pytest
import torch

import slic_ref as SR
import split_merge_ref as M
from raw_calls import same_bytes
from split_merge_calls import NAMES
from test_split_pipeline import NSEG, SIZE, SPLIT, _discs, _model, _same_dict, _threshold, fixed_row_order      # noqa: F401 (the fixture)

MERGE = (1, 4)                                                # (a low bar: the painted masks' parts have shallow saddles)
MERGED = dict(SPLIT, merge=MERGE)


def _numpy(out):
    return {k: out[k].cpu().numpy() for k in NAMES}


def _merged_of(instance_labels, split_labels, prob, got_records, got_labels, got_counts, split_counts):
    """The pipeline's merged keys of some images against ``merge_parts`` on the unmerged run's split labels."""
    from camouflage_multimodal_amd import split as S
    ours = S.merge_parts(instance_labels, split_labels, prob, MERGE)
    assert torch.equal(ours["labels"], got_labels) and torch.equal(ours["counts"], got_counts)
    assert S.split_records(ours["table"], split_counts, *instance_labels.shape[1:], ours["counts"]) == got_records
    return ours


@pytest.mark.gpu
@pytest.mark.parametrize("growth", ["euclidean", "geodesic"])
def test_split_instances_with_merge_is_the_two_calls(growth):
    from camouflage_multimodal_amd import split as S
    from test_split_merge import case, want
    name = "lobe_euclid_4_5" if growth == "euclidean" else "lobe_geo_4_5"
    lab, parts, merge, rows = case(name)
    t = torch.from_numpy(np.array(lab)).cuda()
    plain = S.split_instances(t, None, (7, 10), growth=growth)
    none = S.split_instances(t, None, (7, 10), growth=growth, merge=None)
    assert sorted(plain) == sorted(none) and np.array_equal(plain["labels"].cpu().numpy(), parts)
    same_bytes(_numpy(none), _numpy(plain), "merge=None is today's call", NAMES)
    both = S.split_instances(t, None, (7, 10), growth=growth, merge=merge)
    assert set(both) - set(plain) == {"merge_counts"} and torch.equal(both["counts"], plain["counts"])
    ours = S.merge_parts(t, plain["labels"], None, merge)
    assert torch.equal(both["labels"], ours["labels"]) and torch.equal(both["table"], ours["table"]) and torch.equal(both["merge_counts"], ours["counts"])
    same_bytes({"labels": both["labels"].cpu().numpy(), "table": both["table"].cpu().numpy(), "counts": both["merge_counts"].cpu().numpy()}, want(name), name, NAMES)
    rec, = S.split_records(both["table"], both["counts"], 64, 120, both["merge_counts"])
    assert rec["count"] == 2 and rec["split"] == 1 and rec["parts"] == 3 and rec["merged_groups"] == 1 and [i["area"] for i in rec["instances"]] == [1226, 1722]
    found = S.split_detected(t, None, S.split_options({"merge": merge, "max_instances": 1, "growth": growth}))
    assert found["table"].shape[1] == 2 and found["instances"] == [rec] and torch.equal(found["labels"], both["labels"])      # re-sized from K'' = 2, not K' = 3


@pytest.mark.gpu
def test_detectors_and_the_tuner_with_merge(fixed_row_order):
    from camouflage_multimodal_amd import RegionGraphFineTuner, detect_camouflage, detect_camouflage_batch, detect_camouflage_ragged, encode_instances
    from camouflage_multimodal_amd.instance_match import ground_truth_labels, match_detected, match_options
    m = _model()
    tuner = RegionGraphFineTuner(m, lr=1e-3, seed=5)
    m.eval()
    H, W = 64, 96
    img = torch.from_numpy(np.stack([SR.noise_image(H, W, 20 + i) for i in range(2)])).cuda()
    gt = torch.from_numpy(np.stack([_discs(H, W), _discs(H, W)])).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(n_segments=NSEG, threshold=thr, instances=True, match=True, rle=True)
    base = detect_camouflage_batch(m, img, gt, split=SPLIT, **kw)
    _same_dict(detect_camouflage_batch(m, img, gt, split=dict(SPLIT, merge=None), **kw), base)
    out = detect_camouflage_batch(m, img, gt, split=MERGED, **kw)
    assert set(out) - set(base) == {"split_merge_counts"}
    for k in base:
        if k != "graphs" and k not in ("split_instances", "split_labels", "instance_match", "instance_match_tables", "instance_rles"):
            _same_dict({k: out[k]}, {k: base[k]})
    ours = _merged_of(out["instance_labels"], base["split_labels"], out["prob_maps"][:, 0], out["split_instances"], out["split_labels"],
                      out["split_merge_counts"], out["split_counts"])
    counts = out["split_merge_counts"].tolist()
    assert all(c[1] == k for c, k in zip(counts, base["split_counts"][:, 0].tolist())) and all(c[0] <= c[1] for c in counts), counts
    records, _ = match_detected(out["split_labels"], ours["table"], ground_truth_labels(gt), match_options(True))
    assert out["instance_match"] == records and out["instance_rles"] == encode_instances(out["split_labels"])
    assert [len(r) for r in out["instance_rles"]] == [c[0] for c in counts]
    one = detect_camouflage(m, img[0], gt[0], n_segments=NSEG, threshold=thr, instances=True, split=MERGED)
    assert torch.equal(one["split_labels"][0], out["split_labels"][0]) and torch.equal(one["split_merge_counts"][0], out["split_merge_counts"][0])

    ev = tuner.evaluate(img, gt, instances=True, match=True, split=MERGED, n_segments=NSEG, threshold=thr)
    assert set(ev) == {"metrics", "instances", "split_instances", "instance_match"}
    assert ev["split_instances"] == out["split_instances"] and ev["instance_match"] == out["instance_match"]

    shapes = ((48, 80), (120, 100), (48, 80))                      # two native sizes; the first and the third share a call
    images = [np.rint(SR.noise_image(h, w, 50 + i) * 255).astype(np.uint8) for i, (h, w) in enumerate(shapes)]
    masks = [_discs(h, w) for h, w in shapes]
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match={"thresholds": [0.5, 0.75]})
    plain = detect_camouflage_ragged(m, images, masks, split=SPLIT, **kw)
    rag = detect_camouflage_ragged(m, images, masks, split=MERGED, **kw)
    assert set(rag) - set(plain) == {"split_merge_counts_native"}
    for i, (h, w) in enumerate(shapes):
        labels = rag["instance_labels_native"][i]
        assert tuple(rag["split_labels_native"][i].shape) == (h, w) and tuple(rag["split_merge_counts_native"][i].shape) == (4,)
        ours = _merged_of(labels[None], plain["split_labels_native"][i][None], rag["prob_maps_native"][i][None], [rag["split_instances_native"][i]],
                          rag["split_labels_native"][i][None], rag["split_merge_counts_native"][i][None], rag["split_counts_native"][i][None])
        gt_labels = ground_truth_labels(torch.from_numpy(masks[i]).cuda()[None])
        assert [rag["instance_match"][i]] == match_detected(ours["labels"], ours["table"], gt_labels, match_options({"thresholds": [0.5, 0.75]}))[0]
    er = tuner.evaluate_ragged(images, masks, split=MERGED, **kw)
    assert er["split_instances"] == rag["split_instances_native"] and er["instance_match"] == rag["instance_match"]
    joined = sum(c[2] for c in counts) + sum(int(c[2]) for c in rag["split_merge_counts_native"])
    assert joined >= 1, (counts, [c.tolist() for c in rag["split_merge_counts_native"]])      # some parts are joined, so the merged keys differ


def test_merge_argument_errors_reach_the_entry_points():
    """``ValueError`` before anything touches the device: the model and the images stay on the CPU."""
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage_batch, detect_camouflage_ragged
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).eval()
    img, gt = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, dtype=torch.uint8)
    for bad in ((5, 4), 0.8, (0, 4)):
        with pytest.raises(ValueError, match="^merge"):
            detect_camouflage_batch(m, img, gt, device="cpu", instances=True, split={"merge": bad})
        with pytest.raises(ValueError, match="^merge"):
            detect_camouflage_ragged(m, [np.zeros((8, 8, 3), np.uint8)], [np.zeros((8, 8), np.uint8)], device="cpu", instances=True, split={"merge": bad})
    with pytest.raises(ValueError, match="split needs instances=True"):
        detect_camouflage_batch(m, img, gt, device="cpu", split={"merge": (4, 5)})
    assert M.COUNTS == 4
