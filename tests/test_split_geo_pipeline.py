"""``growth="geodesic"`` from ``split.split_instances`` up through the detector entry points and ``RegionGraphFineTuner.evaluate``
(camouflage_multimodal_amd/split.py, pipeline.py, rg_finetune.py).  The model, the images and the row order of the
CSR are those of tests/test_split_pipeline.py; the spiral is tests/test_split_geo.py's."""
import numpy as np
import pytest
import torch

import slic_ref as SR
from raw_calls import same_bytes
from test_split_geo import NAMES, case, euclid, want
from test_split_pipeline import NSEG, SIZE, _discs, _model, _threshold, fixed_row_order      # noqa: F401 (the fixture)

SPLIT = {"ratio": (1, 2), "max_split": 8, "growth": "geodesic"}


def _numpy(out):
    return {k: out[k].cpu().numpy() for k in NAMES}


def _geodesic_of(labels, prob, got_records, got_labels, got_counts):
    """The pipeline's split keys of some images against ``split_instances(growth="geodesic")`` on their own labels."""
    from camouflage_multimodal_amd import split as S
    o = S.split_options(SPLIT)
    ours = S.split_instances(labels, prob, o["ratio"], o["min_core"], o["max_split"], o["max_instances"], growth="geodesic")
    assert torch.equal(ours["labels"], got_labels) and torch.equal(ours["counts"], got_counts)
    assert S.split_records(ours["table"], ours["counts"], *labels.shape[1:]) == got_records
    return ours


@pytest.mark.gpu
def test_split_instances_growth_on_the_spiral():
    from camouflage_multimodal_amd import split as S
    lab, p = case("spiral")
    t = torch.from_numpy(np.array(lab)).cuda()
    plain = S.split_instances(t, None, p["ratio"], p["min_core"], p["max_split"], p["rows"])
    named = S.split_instances(t, None, p["ratio"], p["min_core"], p["max_split"], p["rows"], growth="euclidean")
    assert sorted(plain) == sorted(named) == ["counts", "labels", "table"]
    same_bytes(_numpy(named), _numpy(plain), "growth='euclidean' is the default call", NAMES)
    same_bytes(_numpy(plain), euclid("spiral"), "euclidean", NAMES)
    geo = S.split_instances(t, None, p["ratio"], p["min_core"], p["max_split"], p["rows"], growth="geodesic")
    same_bytes(_numpy(geo), want("spiral"), "geodesic", NAMES)
    assert geo["rounds"] in (4, 12, 28, 60) and not torch.equal(geo["labels"], plain["labels"])      # 2 x 2 tiles: 4 rounds, then 8, 16, 32 more
    slow = S.split_instances(t[0], None, p["ratio"], p["min_core"], p["max_split"], p["rows"], growth="geodesic", rounds=1)
    same_bytes(_numpy(slow), want("spiral"), "from one round, doubled until nothing is pending", NAMES)
    assert slow["rounds"] in (1, 3, 7, 15, 31)
    found = S.split_detected(t, None, S.split_options({"growth": "geodesic", "rounds": 2, "max_instances": 1}))
    assert found["table"].shape[1] == 2 and found["instances"][0]["count"] == 2 and torch.equal(found["labels"], geo["labels"])


@pytest.mark.gpu
def test_detectors_and_the_tuner_with_geodesic_growth(fixed_row_order):
    from camouflage_multimodal_amd import RegionGraphFineTuner, detect_camouflage_batch, detect_camouflage_ragged
    from camouflage_multimodal_amd.instance_match import ground_truth_labels, match_detected, match_options
    m = _model()
    tuner = RegionGraphFineTuner(m, lr=1e-3, seed=5)
    m.eval()
    H, W = 64, 96
    img = torch.from_numpy(np.stack([SR.noise_image(H, W, 20 + i) for i in range(2)])).cuda()
    gt = torch.from_numpy(np.stack([_discs(H, W), _discs(H, W)])).cuda()
    thr = _threshold(detect_camouflage_batch(m, img, gt, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(n_segments=NSEG, threshold=thr, instances=True, match=True)
    out = detect_camouflage_batch(m, img, gt, split=SPLIT, **kw)
    ours = _geodesic_of(out["instance_labels"], out["prob_maps"][:, 0], out["split_instances"], out["split_labels"], out["split_counts"])
    assert int(out["split_counts"][:, 1].sum()) >= 1, out["split_counts"].tolist()
    records, _ = match_detected(out["split_labels"], ours["table"], ground_truth_labels(gt), match_options(True))
    assert out["instance_match"] == records

    ev = tuner.evaluate(img, gt, instances=True, match=True, split=SPLIT, n_segments=NSEG, threshold=thr)
    assert set(ev) == {"metrics", "instances", "split_instances", "instance_match"}
    assert ev["split_instances"] == out["split_instances"] and ev["instance_match"] == out["instance_match"] and ev["instances"] == out["instances"]
    on = tuner.evaluate(img, gt, instances=True, match=True, split=True, n_segments=NSEG, threshold=thr)
    assert on["split_instances"] == detect_camouflage_batch(m, img, gt, split=True, **kw)["split_instances"]
    base = detect_camouflage_batch(m, img, gt, **kw)
    for off in (tuner.evaluate(img, gt, instances=True, match=True, n_segments=NSEG, threshold=thr),
                tuner.evaluate(img, gt, instances=True, match=True, split=None, n_segments=NSEG, threshold=thr)):
        assert set(off) == {"metrics", "instances", "instance_match"} and off["instance_match"] == base["instance_match"] and off["instances"] == base["instances"]

    shapes = ((48, 80), (120, 100), (48, 80))                      # two native sizes; the first and the third share a call
    images = [np.rint(SR.noise_image(h, w, 50 + i) * 255).astype(np.uint8) for i, (h, w) in enumerate(shapes)]
    masks = [_discs(h, w) for h, w in shapes]
    thr = _threshold(detect_camouflage_ragged(m, images, masks, size=SIZE, n_segments=NSEG)["prob_maps"][:, 0])
    kw = dict(size=SIZE, n_segments=NSEG, threshold=thr, instances=True, match={"thresholds": [0.5, 0.75]})
    rag = detect_camouflage_ragged(m, images, masks, split=SPLIT, **kw)
    assert sum(int(c[1]) for c in rag["split_counts_native"]) >= 1
    for i, (h, w) in enumerate(shapes):
        labels = rag["instance_labels_native"][i]
        ours = _geodesic_of(labels[None], rag["prob_maps_native"][i][None], [rag["split_instances_native"][i]], rag["split_labels_native"][i][None],
                            rag["split_counts_native"][i][None])
        gt_labels = ground_truth_labels(torch.from_numpy(masks[i]).cuda()[None])
        assert [rag["instance_match"][i]] == match_detected(ours["labels"], ours["table"], gt_labels, match_options({"thresholds": [0.5, 0.75]}))[0]
    er = tuner.evaluate_ragged(images, masks, split=SPLIT, **kw)
    assert set(er) == {"metrics", "instances", "split_instances", "instance_match"}
    assert er["split_instances"] == rag["split_instances_native"] and er["instance_match"] == rag["instance_match"]
    assert set(tuner.evaluate_ragged(images, masks, **kw)) == {"metrics", "instances", "instance_match"}
