"""Host-side mirror of the reference API, checked on CPU (no compute calls: the product path has
no CPU fallback and must say so)."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from oracle import params as OP


def test_shared_library_exports_every_declared_symbol():
    """(The declared names, their prototypes and the exports of all ten headers: tests/test_abi_binding.py.)"""
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_fusion.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "run `python -m camouflage_multimodal_amd.build` first"
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.camo_abi_version.restype = ctypes.c_int
    assert L.camo_abi_version() == _lib.ABI_VERSION
    assert f"#define CAMO_ABI_VERSION {_lib.ABI_VERSION}" in hdr
    assert f"#define CAMO_SUMSQ_FLOATS {_lib.SUMSQ_FLOATS}" in hdr
    hdr2 = open(os.path.join(ROOT, "include", "camo_rg_gnn.h")).read()
    assert f"CAMO_RG_NPARAMS" in hdr2 and _lib.RG_NPARAMS == 28
    hdr3 = open(os.path.join(ROOT, "include", "camo_rg_features.h")).read()
    assert f"#define CAMO_RG_MAX_LABELS {_lib.RG_MAX_LABELS}" in hdr3


def test_argument_validation_without_a_gpu():
    """Size/argument checks run on the host before any launch: exercise them through the ABI."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    d = _lib.CamoDims(128, 128, 256, 8, 2, _lib.FUSION_CROSS_ATTENTION, 0.3)
    n = L.camo_workspace_bytes(ctypes.byref(d), 16, 7700, 13)
    assert 100e6 < n < 400e6
    assert L.camo_workspace_bytes(ctypes.byref(d), 1, 1, 1) > 0
    assert L.camo_workspace_bytes(ctypes.byref(d), 0, 10, 13) == 0 and b"B >= 1" in L.camo_last_error()
    bad = _lib.CamoDims(128, 128, 250, 8, 2, 0, 0.3)
    assert L.camo_workspace_bytes(ctypes.byref(bad), 4, 100, 13) == 0 and b"divisible" in L.camo_last_error()
    assert L.camo_workspace_bytes(ctypes.byref(d), 4, 100, 100) == 0 and b"attention kernels" in L.camo_last_error()
    late = _lib.CamoDims(128, 128, 256, 8, 2, _lib.FUSION_LATE, 0.3)
    assert 0 < L.camo_workspace_bytes(ctypes.byref(late), 16, 7700, 13) < 1e6
    assert L.camo_forward(ctypes.byref(d), None, None, None, None, None, 4, 100, 13, 50, None, 0, None, None, None,
                          0, 0, 0, 0, None) == -1
    # camo_forward_cached: a promise without a buffer, a misaligned buffer (both refused before anything is dereferenced)
    st = ctypes.c_int32(7)
    assert L.camo_forward_cached(ctypes.byref(d), None, None, None, None, None, 4, 100, 13, 50, None, 0, None, None, None,
                                 0, 0, 1, 1, None, 1, ctypes.byref(st), None) == -1 and b"shadows_valid" in L.camo_last_error() and st.value == 0
    assert L.camo_forward_cached(ctypes.byref(d), None, None, None, None, None, 4, 100, 13, 50, None, 0, None, None, None,
                                 0, 0, 1, 1, ctypes.c_void_p(0x1010), 0, None, None) == -1 and b"256-byte" in L.camo_last_error()
    # ... and a call that would save for camo_backward (no CAMO_FWD_INFERENCE): the backward could not find the transposed shadows
    assert L.camo_forward_cached(ctypes.byref(d), None, None, None, None, None, 4, 100, 13, 50, None, 0, None, None, None,
                                 1, 0, 1, 0, ctypes.c_void_p(0x1000), 0, None, None) == -2 and b"inference calls only" in L.camo_last_error()
    assert L.camo_shadow_bytes(ctypes.byref(d)) % 256 == 0 and L.camo_shadow_bytes(ctypes.byref(d)) > 3e6 and L.camo_shadow_bytes(ctypes.byref(bad)) == 0
    assert L.camo_batch_desc_bytes(16, 7700) >= 4 * (7700 + 16 + 17) and L.camo_batch_desc_bytes(0, 5) == 0
    assert L.camo_loss(None, None, None, None, 4, 2, None, None, None, None, None) == -1


def test_module_surface_matches_reference():
    from camouflage_multimodal_amd import MultimodalCamouflageDetector, build_multimodal_model
    m = build_multimodal_model({})
    assert [k for k, _ in OP.param_specs()] == list(m.state_dict().keys())
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: s for k, s in OP.param_specs()}
    assert sum(p.numel() for p in m.parameters()) == 1448710
    for cfg in (dict(fusion_type="late"), dict(rg_dim=64, kg_dim=64, hidden_dim=64, num_heads=2), dict(num_classes=5)):
        mm = build_multimodal_model(cfg)
        assert [k for k, _ in OP.param_specs(cfg)] == list(mm.state_dict().keys())
    assert m.config == dict(rg_dim=128, kg_dim=128, hidden_dim=256, num_heads=8, fusion_type="cross_attention",
                            num_classes=2, dropout=0.3)
    with pytest.raises(ValueError, match="Unknown fusion_type: nope"):
        MultimodalCamouflageDetector(fusion_type="nope")
    # state_dict round trip (strict) keeps the flat buffer coherent
    sd = {k: torch.from_numpy(v) for k, v in OP.make_params({}, 3).items()}
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k])
    flat = m._engine.flat_params
    for p in m.parameters():
        assert flat.data_ptr() <= p.data_ptr() < flat.data_ptr() + 4 * flat.numel() and p.data_ptr() % 16 == 0
    # torch's default initialisation of the corresponding reference modules
    fresh = build_multimodal_model({})
    assert float(fresh.fusion.cross_attn_rg2kg.in_proj_bias.detach().abs().max()) == 0.0
    assert float(fresh.fusion.cross_attn_rg2kg.out_proj.bias.detach().abs().max()) == 0.0
    assert torch.equal(fresh.fusion.ln_rg.weight, torch.ones(256))
    bound = np.sqrt(6.0 / (256 + 768))
    assert float(fresh.fusion.cross_attn_kg2rg.in_proj_weight.detach().abs().max()) <= bound + 1e-6


def test_no_cpu_fallback_and_reference_errors():
    from camouflage_multimodal_amd import NativeTrainer, build_multimodal_model
    from camouflage_multimodal_amd._lib import CamoError
    m = build_multimodal_model({})
    with pytest.raises(CamoError, match="no CPU fallback"):
        m(torch.zeros(1, 5, 128), torch.zeros(1, 13, 128))
    with pytest.raises(ValueError, match="rg_embeddings must be 2D/3D/4D tensor"):
        m(torch.zeros(1, 1, 1, 5, 128), torch.zeros(1, 13, 128))
    with pytest.raises(ValueError, match="kg_embeddings must be 2D/3D/4D tensor"):
        m(torch.zeros(1, 5, 128), torch.zeros(13))
    with pytest.raises(CamoError, match="no CPU fallback"):
        NativeTrainer(m).step(torch.zeros(5, 128), [5], torch.zeros(1, 13, 128), torch.zeros(1, dtype=torch.long),
                              torch.zeros(1), torch.zeros(1))
    # nothing under the package imports the oracle
    pkg = os.path.join(ROOT, "camouflage_multimodal_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, f)).read(), f


def test_losses_metrics_and_schedule_against_golden():
    from camouflage_multimodal_amd import AggressiveFocalLoss, calculate_f1_score, cosine_warm_restarts_lr
    g = load_golden("loss")
    x = torch.from_numpy(g["logits"]).requires_grad_(True)
    l = AggressiveFocalLoss(0.75, 3.0)(x, torch.from_numpy(g["targets"]))
    l.backward()
    assert abs(float(l) - float(g["focal"])) < 1e-6
    assert np.abs(x.grad.numpy() - g["focal_grad"]).max() < 1e-6
    f = calculate_f1_score(torch.from_numpy(g["f1_pred"]), torch.from_numpy(g["f1_lab"]))
    for k, v in f.items():
        assert abs(float(v) - float(g[f"f1/{k}"])) < 1e-6, k
    lrs = [cosine_warm_restarts_lr(5e-4, ep) for ep in range(35)]
    assert np.abs(np.array(lrs) - g["lr_schedule"]).max() < 1e-9


def test_pack_samples_and_embedding_matcher(kg_real):
    from camouflage_multimodal_amd import EmbeddingMatcher, pack_samples
    names = [str(n) for n in load_golden("kg_embeddings")["names"]]
    kg = {n: torch.from_numpy(kg_real[i:i + 1].copy()) for i, n in enumerate(names)}
    rg = {f"COD10K-CAM-1-Aquatic-{i}-{org}-{i}.jpg": {"node_embeddings": torch.from_numpy(OP.make_rg(5 + i, 128, seed=i)),
                                                       "graph_embedding": torch.zeros(1, 128), "num_nodes": 5 + i}
          for i, org in enumerate(["BatFish", "Bird", "Crab"])}
    em = EmbeddingMatcher(rg_embeddings=rg, kg_embeddings=kg)
    assert em.extract_category_from_filename("COD10K-CAM-1-Aquatic-1-BatFish-1.jpg") == "Fish"       # substring match
    assert em.extract_category_from_filename("COD10K-CAM-2-Terrestrial-1-Bird-7.jpg") == "Bird"      # exact match
    assert em.extract_category_from_filename("COD10K-CAM-1-Aquatic-3-Crab-3.jpg") is None
    assert em.extract_category_from_filename("short-name.jpg") is None
    matched = em.create_matched_dataset(use_all_kg_categories=True)
    assert len(matched) == 3 and matched[0]["kg_embeddings"].shape == (13, 1, 128) and matched[2]["num_rg_nodes"] == 7
    assert matched[0]["category_ids"] == list(range(13))
    one = em.create_matched_dataset(use_all_kg_categories=False)
    assert one[0]["kg_embeddings"].shape == (1, 1, 128) and one[0]["category_ids"] == [names.index("Fish")]
    assert one[2]["category_ids"] == [0] and torch.allclose(one[2]["kg_embeddings"][0, 0], torch.from_numpy(kg_real).mean(0))
    batch = [dict(rg_node_emb=s["rg_node_embeddings"], kg_emb=s["kg_embeddings"], mask_label=i % 2, edge_label=1.0,
                  score_label=0.25 * i) for i, s in enumerate(matched)]
    rgp, nrs, kgp, y, e, sc = pack_samples(batch, "cpu")
    assert nrs == [5, 6, 7] and rgp.shape == (18, 128) and kgp.shape == (3, 13, 128)
    assert torch.equal(rgp[5:11], matched[1]["rg_node_embeddings"]) and y.tolist() == [0, 1, 0] and sc.tolist() == [0.0, 0.25, 0.5]


def test_device_resident_dataset_batches_on_cpu():
    from camouflage_multimodal_amd import DeviceResidentDataset
    samples = [dict(rg_node_emb=torch.from_numpy(OP.make_rg(3 + i, 128, seed=i)), kg_emb=torch.from_numpy(OP.make_kg(13, 128, seed=i))[:, None, :],
                    mask_label=i % 2, edge_label=float(i % 2), score_label=0.1 * i) for i in range(5)]
    ds = DeviceResidentDataset(samples, "cpu")
    rg, nrs, kg, y, e, s = ds.batch([4, 1])
    assert nrs == [7, 4] and rg.shape == (11, 128) and kg.shape == (2, 13, 128)
    assert torch.equal(rg[:7], samples[4]["rg_node_emb"]) and torch.equal(rg[7:], samples[1]["rg_node_emb"])
    assert y.tolist() == [0, 1] and abs(float(s[0]) - 0.4) < 1e-7
    aug = DeviceResidentDataset(samples, "cpu", augment=True, seed=1)
    diffs = [float((aug.batch([i])[0] - samples[i]["rg_node_emb"]).abs().max()) for i in range(5) for _ in range(4)]
    assert any(d == 0.0 for d in diffs) and any(0 < d < 0.1 for d in diffs)      # noise with probability 1/2, sigma 0.01


def test_checkpoint_format_interchanges_with_torch_adamw(tmp_path):
    """The optimizer state this package writes loads into torch.optim.AdamW over the same parameter
    list (what a reference user resuming from a checkpoint would do), and the checkpoint dict has the
    reference's keys (train_multimodal.py:464-474)."""
    from camouflage_multimodal_amd import FusedClipAdamW, build_multimodal_model, load_multimodal_model
    from camouflage_multimodal_amd.train_multimodal import save_best_checkpoint

    class T:  # minimal stand-in for NativeTrainer: the checkpoint writer only touches .opt
        pass
    cfg = {"model": dict(rg_dim=16, kg_dim=16, hidden_dim=32, num_heads=4), "learning_rate": 5e-4}
    m = build_multimodal_model(cfg["model"])
    t = T(); t.opt = FusedClipAdamW(m)
    t.opt._state()[0].uniform_(-1, 1); t.opt._state()[1].uniform_(0, 1); t.opt.step_count = 7
    path = os.path.join(tmp_path, "multimodal_best_fixed.pth")
    save_best_checkpoint(path, m, t, 3, 0.5, {"f1_class_1": torch.tensor(0.75), "f1_avg": torch.tensor(0.7)}, 80.0, 60.0, cfg)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "val_f1_class_1", "val_f1_avg",
                       "val_acc_0", "val_acc_1", "config"}
    ref_opt = torch.optim.AdamW(build_multimodal_model(cfg["model"]).parameters(), lr=5e-4, weight_decay=1e-4)
    ref_opt.load_state_dict(ck["optimizer_state_dict"])
    st = ref_opt.state_dict()["state"]
    assert len(st) == len(list(m.parameters())) and float(st[0]["step"]) == 7.0
    m2, cfg2 = load_multimodal_model(path, "cpu")
    assert cfg2 == cfg and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    # and back: a torch AdamW state loads into the fused optimizer
    o2 = FusedClipAdamW(m2); o2.load_state_dict(ref_opt.state_dict())
    a, b = o2.state_dict()["state"], t.opt.state_dict()["state"]
    assert o2.step_count == 7 and all(torch.equal(a[i]["exp_avg"], b[i]["exp_avg"]) and torch.equal(a[i]["exp_avg_sq"], b[i]["exp_avg_sq"]) for i in a)


def test_build_ordered_kg_tensor():
    from camouflage_multimodal_amd import build_ordered_kg_tensor
    kg = {"b": torch.ones(1, 4), "a": torch.zeros(1, 4), "c": torch.full((1, 4), 2.0)}
    t, od = build_ordered_kg_tensor(kg)
    assert list(od) == ["a", "b", "c"] and t.shape == (3, 1, 4) and t[:, 0, 0].tolist() == [0.0, 1.0, 2.0]
    t2, od2 = build_ordered_kg_tensor(torch.arange(6.0).view(3, 2))
    assert list(od2) == ["cat_0", "cat_1", "cat_2"] and t2.shape == (3, 2)


def _write_png(path, arr):
    from PIL import Image
    Image.fromarray(arr.astype(np.uint8), mode="L").save(path)


def test_smart_dataset_labels_weights_and_png_labels(tmp_path):
    """Data glue of train_multimodal.py:62-188 on synthetic ground-truth PNGs: the label rule (mean intensity > 0.1 and
    more than 5 % of the pixels above 10), edge_label = float(edge.mean() > 10), score_label = mask.mean()/255, and
    the aggressive sample weights (majority/count * 5 for class 1, times the confidence) feeding the sharded sampler."""
    from camouflage_multimodal_amd import SmartMultimodalDataset, extract_label_from_mask
    from camouflage_multimodal_amd.ddp import sharded_weighted_sampler
    from camouflage_multimodal_amd.train_multimodal import png_labels
    dirs = {k: tmp_path / k for k in ("gt_object", "gt_instance", "gt_edge")}
    for d in dirs.values():
        d.mkdir()
    rs = np.random.RandomState(0)
    masks = {}
    blob = np.zeros((256, 320)); blob[40:200, 60:260] = 255                  # one big object: label 1
    masks["a"] = blob
    masks["b"] = np.zeros((64, 80))                                          # empty: label 0
    tiny = np.zeros((64, 80)); tiny[0:3, 0:3] = 255                          # < 5 % of the pixels: label 0
    masks["c"] = tiny
    many = np.zeros((64, 80))
    for i in range(12):                                                      # 12 separate blobs (> 10 contours)
        many[4 * (i // 6) * 8 + 2:4 * (i // 6) * 8 + 22, 13 * (i % 6) + 1:13 * (i % 6) + 11] = 200
    masks["d"] = many
    edges = {"a": np.full((64, 80), 30.0), "b": np.zeros((64, 80)), "c": np.full((64, 80), 10.0), "d": np.full((64, 80), 11.0)}
    matched = []
    for name, m in masks.items():
        _write_png(dirs["gt_object"] / f"{name}.png", m); _write_png(dirs["gt_instance"] / f"{name}.png", m)
        _write_png(dirs["gt_edge"] / f"{name}.png", edges[name])
        matched.append({"image_name": name + ".jpg", "rg_node_embeddings": torch.from_numpy(OP.make_rg(4, 128, seed=1)),
                        "kg_embeddings": torch.zeros(13, 1, 128)})
    matched.append({"image_name": "missing.jpg", "rg_node_embeddings": torch.zeros(2, 128), "kg_embeddings": torch.zeros(13, 1, 128)})
    ds = SmartMultimodalDataset(matched, str(dirs["gt_object"]), str(dirs["gt_instance"]), str(dirs["gt_edge"]))
    assert len(ds) == 4 and ds.get_labels() == [1, 0, 0, 1]
    mean_a, mean_d = masks["a"].mean() / 255, masks["d"].mean() / 255
    conf = [s["confidence"] for s in ds.valid_samples]
    assert abs(conf[0] - min(2 * mean_a, 1.0)) < 1e-12            # a clean blob has few edge pixels (< 2 %): doubled confidence
    assert abs(conf[1] - 1.0) < 1e-12 and abs(conf[2] - (1 - masks["c"].mean() / 255)) < 1e-12
    assert abs(conf[3] - min(2 * mean_d, 1.0)) < 1e-12            # 12 external contours > 10
    assert extract_label_from_mask(str(tmp_path / "nope.png")) == (0, 0.0)
    small = np.zeros((64, 80)); small[10:50, 20:70] = 255                     # same shape at 64x80: its outline is 3.5 % of the
    _write_png(tmp_path / "small.png", small)                                 # pixels (>= 2 %) and it is one contour: plain mean
    assert extract_label_from_mask(str(tmp_path / "small.png")) == (1, small.mean() / 255)
    item = ds[0]
    assert set(item) == {"rg_node_emb", "kg_emb", "mask_label", "confidence", "edge_label", "score_label", "image_name"}
    assert item["edge_label"] == 1.0 and abs(item["score_label"] - mean_a) < 1e-12
    assert ds[2]["edge_label"] == 0.0 and ds[3]["edge_label"] == 1.0          # mean 10 is not > 10; 11 is
    assert png_labels(str(dirs["gt_object"] / "b.png"), str(dirs["gt_edge"] / "b.png")) == (0.0, 0.0)
    w = ds.get_aggressive_sample_weights()                                    # counts {1: 2, 0: 2}: majority 2
    assert np.allclose(w, [5.0 * conf[0], conf[1], conf[2], 5.0 * conf[3]])
    draw0 = sharded_weighted_sampler(w, 64, epoch=1, world=2, rank=0, seed=3)
    draw1 = sharded_weighted_sampler(w, 64, epoch=1, world=2, rank=1, seed=3)
    assert len(draw0) == len(draw1) == 32 and sum(ds.get_labels()[i] for i in draw0 + draw1) > 40    # class 1 oversampled
    assert [s["mask_label"] for s in ds.training_samples()] == [1, 0, 0, 1]


def test_deepcopy_and_pickle_give_the_copy_its_own_engine():
    import copy
    from camouflage_multimodal_amd import build_multimodal_model
    m = build_multimodal_model(dict(rg_dim=16, kg_dim=16, hidden_dim=32, num_heads=4))
    c = copy.deepcopy(m)
    assert c._engine.module() is c and m._engine.module() is m
    fc, fm = c._engine.flat_params, m._engine.flat_params
    assert fc.data_ptr() != fm.data_ptr() and torch.equal(fc, fm)
    for p in c.parameters():
        assert fc.data_ptr() <= p.data_ptr() < fc.data_ptr() + 4 * fc.numel()
    with torch.no_grad():
        next(c.parameters()).add_(1.0)                       # updating the copy leaves the original alone
    assert not torch.equal(c._engine.flat_params, m._engine.flat_params)
    buf = io.BytesIO()
    torch.save(m, buf); buf.seek(0)
    m2 = torch.load(buf, weights_only=False)                 # (a file this test wrote itself)
    assert m2._engine.module() is m2 and torch.equal(m2._engine.flat_params, fm)


def test_device_and_label_checks_run_before_the_abi(monkeypatch):
    from camouflage_multimodal_amd import _lib, build_multimodal_model
    from camouflage_multimodal_amd.engine import check_labels
    with pytest.raises(IndexError, match="Target 2 is out of bounds"):
        check_labels(torch.tensor([0, 2, 1]), 2)
    with pytest.raises(IndexError, match="Target -1 is out of bounds"):
        check_labels(torch.tensor([-1]), 2)
    check_labels(torch.tensor([0, 1]), 2)
    m = build_multimodal_model(dict(rg_dim=16, kg_dim=16, hidden_dim=32, num_heads=4))
    monkeypatch.setattr(_lib, "require_device", lambda t, name: None)        # pretend 'cpu' is a HIP device
    with pytest.raises(_lib.CamoError, match="every tensor of a call must live on the model's device"):
        m._engine._same_device(torch.zeros(3, 16, device="meta"), "rg_embeddings")
    assert m._engine._same_device(torch.zeros(3, 16), "rg_embeddings") is not None
    b0 = m._engine._seed_base
    m._engine.fold_rank(0); s0 = m._engine._seed_base
    m._engine.fold_rank(1); s1 = m._engine._seed_base
    assert len({b0, s0, s1}) == 3                                            # ranks draw different dropout streams


def test_device_resident_dataset_batch_index_is_built_without_host_loops():
    """DeviceResidentDataset.batch gathers a minibatch with index arithmetic on the dataset's device (here: the CPU) and hands
    the packed offsets on as ``nrs.offsets_dev``: same rows as the per-sample slices, int32 offsets = cumsum of the counts."""
    import torch
    from camouflage_multimodal_amd import DeviceResidentDataset
    rs = np.random.RandomState(0)
    samples = [dict(rg_node_emb=torch.from_numpy(rs.standard_normal((n, 8)).astype(np.float32)), kg_emb=torch.from_numpy(rs.standard_normal((3, 1, 8)).astype(np.float32)),
                    mask_label=i % 2, edge_label=float(i % 3 == 0), score_label=0.1 * i) for i, n in enumerate([5, 1, 7, 3, 4, 2])]
    ds = DeviceResidentDataset(samples, "cpu")
    idx = [4, 1, 1, 5, 0]
    rg, nrs, kg, y, e, s = ds.batch(idx)
    assert list(nrs) == [4, 1, 1, 2, 5] and nrs.offsets_dev.dtype == torch.int32 and nrs.offsets_dev.tolist() == [0, 4, 5, 6, 8, 13]
    assert torch.equal(rg, torch.cat([samples[i]["rg_node_emb"] for i in idx]))
    assert torch.equal(kg, torch.stack([samples[i]["kg_emb"].reshape(3, 8) for i in idx]))
    assert y.tolist() == [0, 1, 1, 1, 0]


def test_schedule_options_are_per_engine_state():
    """VERDICT r3 item 7 / SURVEY 8(b) "no global mutable state": the schedule options live in a caller-owned camo_options_t behind
    camo_dims_t::options.  The Python defaults equal camo_options_init's; two engines hold independent values; the process-wide
    convenience the tests use (engine.set_option_all, reached through the old camo_debug_set_option call shape) is Python state
    applied to every live engine, not library state; unknown names are refused."""
    import ctypes as C
    from camouflage_multimodal_amd import _lib, build_multimodal_model, engine
    L = _lib.lib()
    o = _lib.CamoOptions()
    assert L.camo_options_init(C.byref(o)) == 0
    assert {n: getattr(o, n) for n in _lib.OPTION_NAMES} == _lib.OPTION_DEFAULTS
    assert [f[0] for f in _lib.CamoOptions._fields_] == list(_lib.OPTION_NAMES)
    a, b = build_multimodal_model({}), build_multimodal_model({})
    a._engine.set_option("fused_rt", 4)
    assert a._engine.options.fused_rt == 4 and b._engine.options.fused_rt == -1
    assert a._engine.dims.options.contents.fused_rt == 4                     # (what the library reads)
    try:
        L.camo_debug_set_option(b"wide2", 0)                                 # the tests' call shape: every live engine + later ones
        assert a._engine.options.wide2 == 0 and b._engine.options.wide2 == 0
        c = build_multimodal_model({})
        assert c._engine.options.wide2 == 0 and c._engine.options.fused_rt == -1
    finally:
        L.camo_debug_set_option(b"wide2", -1)
        engine._OPTION_DEFAULTS.clear()
    assert L.camo_options_set(C.byref(o), b"no_such_option", 1) != 0
    with pytest.raises(_lib.CamoError):
        engine.set_option_all("no_such_option", 1)


def test_calls_that_launch_no_tail_leave_the_callers_options_alone():
    """The library reads the caller's options and writes back only the one-shot tail_skip_arrival, once a one-launch tail took it.
    Size queries, the workspace-offset lookup and a forward refused before any launch leave every field as it was."""
    import ctypes as C
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    o = _lib.CamoOptions()
    want = {n: v + 2 for n, v in _lib.OPTION_DEFAULTS.items()}
    want["tail_skip_arrival"] = 6
    for n, v in want.items():
        setattr(o, n, v)
    d = _lib.CamoDims(128, 128, 256, 8, 2, _lib.FUSION_CROSS_ATTENTION, 0.3, C.pointer(o))
    assert L.camo_workspace_bytes(C.byref(d), 16, 7700, 13) > 0
    assert L.camo_shadow_bytes(C.byref(d)) > 0
    assert L.camo_debug_ws_offset(C.byref(d), 16, 7700, 13, b"R16") >= 0
    assert L.camo_forward(C.byref(d), None, None, None, None, None, 4, 100, 13, 50, None, 0, None, None, None,
                          0, 0, 0, 0, None) == -1
    assert {n: getattr(o, n) for n in _lib.OPTION_NAMES} == want
