"""Round-2 parity cases ("Next round" item 1): the benchmarked mode against the oracle, the long-sequence
configuration, the epoch loop / validation / checkpoint / history / inference post-processing end to end.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import assert_attention_grad_blocks_close, assert_close
from oracle import fusion_oracle as FO
from oracle import params as OP
from test_hip_parity import make_model, outs6, t2n

pytestmark = pytest.mark.gpu


def _grad_errors(model, ref, coef):
    num = den = 0.0
    rels = []
    for k, p in model.named_parameters():
        want = ref["raw_grads"][k].astype(np.float64); got = t2n(p.grad).astype(np.float64) / coef
        num += ((got - want) ** 2).sum(); den += (want ** 2).sum()
        rels.append((np.sqrt(((got - want) ** 2).sum()) / max(np.sqrt((want ** 2).sum()), 1e-30), np.sqrt((want ** 2).sum()), k))
    rels.sort(reverse=True)
    return np.sqrt(num / den), np.sqrt(den), rels


def test_benchmarked_mode_bf16_dropout_b16_matches_oracle(kg_real):
    """What bench.py times: default configuration, bf16 precision (bf16-resident schedule), train mode with dropout 0.3,
    B = 16 samples drawn from the real Nr histogram -- against the oracle's train step with the same seed, i.e. the same
    counter-hash dropout masks at all nine sites."""
    from camouflage_multimodal_amd import NativeTrainer
    cfg = OP.full_cfg()
    h = load_golden("nr_histogram")
    rs = np.random.RandomState(11)
    nrs = [int(x) for x in rs.choice(h["values"], size=16, p=h["counts"] / h["counts"].sum())]
    rg = [OP.make_rg(n, 128, seed=900 + i) for i, n in enumerate(nrs)]
    kg = np.stack([kg_real] * 16)
    y, e, s = OP.make_labels(16, seed=21)
    dseed = 0x5EEDC0FFEE123457
    m = make_model(cfg, 0, "bf16").train()
    tr = NativeTrainer(m, keep_grads=True)
    # the oracle in its bf16-operand mode: it rounds the tensors the kernels round (oracle/fusion_oracle.py), so what is left
    # between the two is summation order and the one rounding the oracle models statistically (the KG->RG exponentials);
    # the reference-exact f32 oracle bounds the logits (north_star: 1e-3)
    orc32 = FO.FusionOracle(cfg, OP.make_params(cfg, 0))
    ref32, _ = orc32.forward_list(rg, kg, training=True, seed=dseed)
    orc = FO.FusionOracle(cfg, OP.make_params(cfg, 0), bf16_operands=True)
    ref = FO.train_step(orc, FO.AdamW(orc.p), rg, kg, y, e, s, training=True, seed=dseed)
    terms, pred = tr.step(torch.from_numpy(np.concatenate(rg)).cuda(), nrs, torch.from_numpy(kg).cuda(), torch.from_numpy(y),
                          torch.from_numpy(e), torch.from_numpy(s), seed=dseed)
    assert_close(t2n(terms), ref["loss_terms"], 5e-4, 5e-4, "bf16 + dropout loss terms")
    assert (t2n(pred) == outs6(ref["outs"])[:, :2].argmax(1)).all()
    assert (t2n(pred) == outs6(ref32)[:, :2].argmax(1)).all()
    assert_close(t2n(tr.opt.grad_norm())[0], ref["grad_norm"], 0, 5e-3, "grad norm")
    coef = min(1.0, 1.0 / (float(ref["grad_norm"]) + 1e-6))
    tr.engine.ensure_flat_grads(attach=True)
    total, gn, rels = _grad_errors(m, ref, coef)
    print("bf16+dropout B=16: global relative gradient error vs the bf16-operand oracle", total, "worst tensors", [(f"{r:.3f}", f"{n:.2e}", k) for r, n, k in rels[:5]])
    assert total < 2e-3                                                # (measured 4.5e-4; worst tensor ffn_kg.0.weight 0.7 %)
    assert all(r < 1.5e-2 for r, n, _ in rels if n > 1e-3 * gn)
    assert_attention_grad_blocks_close({k: t2n(p.grad) / np.float32(coef) for k, p in m.named_parameters()}, ref["raw_grads"], what="bf16 + dropout, B = 16")


def test_long_sequence_config_nr2048(kg_real):
    """BASELINE configs[3] stand-in: Nr = 2048 nodes per sample, B = 4 -- the KG->RG softmax spans 2048 keys.
    f32: eval logits and one training step against the oracle; bf16: logits within north_star's 1e-3."""
    from camouflage_multimodal_amd import NativeTrainer
    cfg = OP.full_cfg(dict(dropout=0.0))
    nrs = [2048] * 4
    rg = [OP.make_rg(n, 128, seed=1200 + i) for i, n in enumerate(nrs)]
    kg = np.stack([kg_real] * 4)
    y, e, s = OP.make_labels(4, seed=33)
    orc = FO.FusionOracle(cfg, OP.make_params(cfg, 0))
    ref_eval, _ = orc.forward_list(rg, kg)
    rgp = torch.from_numpy(np.concatenate(rg)).cuda(); kgt = torch.from_numpy(kg).cuda()
    m = make_model(cfg, 0, "f32").eval()
    with torch.no_grad():
        o = m.forward_packed(rgp, nrs, kgt, return_attention=True)
    assert_close(np.concatenate([t2n(v) for v in o[:4]], axis=1), outs6(ref_eval), 2e-5, 1e-5, "f32 logits at Nr=2048")
    for b in range(4):
        assert_close(t2n(o[4]["kg2rg"][b]), ref_eval["attn_kg2rg"][b], 2e-7, 2e-4, "kg2rg map over 2048 keys")
        assert_close(t2n(o[4]["kg2rg"][b]).sum(1), np.ones(13), 1e-5, 0, "kg2rg rows sum to 1")
    mb = make_model(cfg, 0, "bf16").eval()
    with torch.no_grad():
        ob = mb.forward_packed(rgp, nrs, kgt)
    err = np.abs(np.concatenate([t2n(v) for v in ob], axis=1) - outs6(ref_eval)).max()
    print("bf16 max |logit err| at Nr=2048 =", err)
    assert err < 1e-3
    m.train()
    tr = NativeTrainer(m, keep_grads=True)
    ref = FO.train_step(orc, FO.AdamW(orc.p), rg, kg, y, e, s, training=True)
    terms, _ = tr.step(rgp, nrs, kgt, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s))
    assert_close(t2n(terms), ref["loss_terms"], 2e-5, 1e-4, "loss terms at Nr=2048")
    assert_close(t2n(tr.opt.grad_norm())[0], ref["grad_norm"], 0, 2e-4, "grad norm at Nr=2048")
    coef = min(1.0, 1.0 / (float(ref["grad_norm"]) + 1e-6))
    tr.engine.ensure_flat_grads(attach=True)
    for k, p in m.named_parameters():
        want = ref["raw_grads"][k]
        rms = float(np.sqrt((want.astype(np.float64) ** 2).mean()))
        assert_close(t2n(p.grad) / coef, want, 4e-4 * rms + 2e-7, 4e-4, f"grad {k} at Nr=2048")


def _synthetic_samples(n, seed0):
    out = []
    for i in range(n):
        y, e, s = OP.make_labels(1, seed=seed0 + i)
        out.append(dict(rg_node_emb=torch.from_numpy(OP.make_rg(20 + 7 * (i % 5), 128, seed=seed0 + i)),
                        kg_emb=torch.from_numpy(OP.make_kg(13, 128, seed=seed0 + 50 + i))[:, None, :],      # [13,1,128] like EmbeddingMatcher
                        mask_label=int(i % 2), edge_label=float(e[0]), score_label=float(s[0]), image_name=f"img{i}.jpg"))
    return out


def test_fit_runs_epochs_validation_checkpoint_and_history(tmp_path):
    """train_multimodal_fixed's epoch loop (train_multimodal.py:397-492) on 12 synthetic samples through
    DeviceResidentDataset: two epochs; validate_fixed's CE / F1 / per-class accuracy against the oracle's eval forward
    on the trained weights; the best-checkpoint file and training_history_fixed.json as the reference writes them."""
    from camouflage_multimodal_amd import DeviceResidentDataset, fit, load_multimodal_model, validate_fixed
    from camouflage_multimodal_amd.optim import cosine_warm_restarts_lr
    torch.manual_seed(0)
    train_s, val_s = _synthetic_samples(12, 100), _synthetic_samples(6, 300)
    tds, vds = DeviceResidentDataset(train_s, "cuda"), DeviceResidentDataset(val_s, "cuda")
    train_loader = [tds.batch(list(range(i, i + 4))) for i in range(0, 12, 4)]
    val_loader = [[val_s[0], val_s[1], val_s[2]], vds.batch([3, 4, 5])]          # reference-style dict lists and packed tuples both work
    cfg = {"model": dict(rg_dim=128, kg_dim=128, hidden_dim=256, num_heads=8, fusion_type="cross_attention", num_classes=2, dropout=0.3),
           "learning_rate": 5e-4, "weight_decay": 1e-4, "epochs": 2, "batch_size": 4, "checkpoint_dir": str(tmp_path / "ckpt"),
           "precision": "f32"}
    logs = []
    model, hist = fit(cfg, train_loader, val_loader, device="cuda", log=logs.append)
    keys = {"train_loss", "val_loss", "train_f1_class_0", "train_f1_class_1", "train_f1_avg", "val_f1_class_0", "val_f1_class_1",
            "val_f1_avg", "val_acc_0", "val_acc_1"}
    assert set(hist) == keys and all(len(v) == 2 for v in hist.values()) and len(logs) == 2
    assert all(np.isfinite(v).all() for v in hist.values()) and hist["train_loss"][0] > 0
    with open(tmp_path / "ckpt" / "training_history_fixed.json") as f:
        assert json.load(f) == hist
    # validation numbers against the oracle on the trained parameters
    sd = {k: t2n(v) for k, v in model.state_dict().items()}
    orc = FO.FusionOracle(cfg["model"], sd)
    ref, _ = orc.forward_list([s["rg_node_emb"].numpy() for s in val_s], np.stack([s["kg_emb"].numpy()[:, 0] for s in val_s]))
    labels = np.array([s["mask_label"] for s in val_s])
    ce = float(np.mean([FO.cross_entropy(ref["mask"][i:i + 1], labels[i:i + 1])[0] for i in range(6)]))
    preds = ref["mask"].argmax(1)
    f1 = FO.f1_scores(preds, labels)
    vl, vf1, a0, a1 = validate_fixed(model, val_loader, "cuda")
    assert abs(vl - ce) < 1e-4 and abs(vl - hist["val_loss"][-1]) < 1e-6
    for k in ("f1_class_0", "f1_class_1", "f1_avg", "precision_1", "recall_1"):
        assert abs(float(vf1[k]) - f1[k]) < 1e-6, k
    assert abs(a0 - 100 * ((preds == labels) & (labels == 0)).sum() / 3) < 1e-9 and abs(a1 - 100 * ((preds == labels) & (labels == 1)).sum() / 3) < 1e-9
    # the best checkpoint (written iff some epoch's class-1 F1 beat 0)
    path = tmp_path / "ckpt" / "multimodal_best_fixed.pth"
    if max(hist["val_f1_class_1"]) > 0:
        ck = torch.load(path, weights_only=True)
        assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "val_f1_class_1", "val_f1_avg", "val_acc_0",
                           "val_acc_1", "config"}
        best = int(np.argmax(hist["val_f1_class_1"]))            # first epoch reaching the maximum is the one saved last
        assert ck["epoch"] == best and abs(ck["val_f1_class_1"] - hist["val_f1_class_1"][best]) < 1e-9 and ck["config"] == cfg
        # the reference saves after scheduler.step(): the stored lr is the next epoch's
        assert abs(ck["optimizer_state_dict"]["param_groups"][0]["lr"] - cosine_warm_restarts_lr(5e-4, best + 1)) < 1e-12
        m2, c2 = load_multimodal_model(str(path), "cuda")
        assert c2 == cfg and not m2.training
    else:
        assert not path.exists()


def test_predict_post_processing_and_batch_results(tmp_path, kg_real):
    """predict_single_image's post-processing (test_multimodal.py:105-150) and batch_results.json (:350-375) against the oracle."""
    from camouflage_multimodal_amd import predict_embedding_directory, predict_from_embeddings
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "f32").eval()
    orc = FO.FusionOracle(cfg, OP.make_params(cfg, 0))
    names = [str(n) for n in load_golden("kg_embeddings")["names"]]
    kgd = {n: torch.from_numpy(kg_real[i:i + 1].copy()) for i, n in enumerate(names)}       # insertion order = category id
    order = sorted(range(13), key=lambda i: names[i])                                       # inference sorts the keys [:65]
    rgs = {f"img{i}.jpg": {"node_embeddings": torch.from_numpy(OP.make_rg(303 + 50 * i, 128, seed=40 + i))} for i in range(3)}
    sm = lambda x: np.exp(x - x.max()) / np.exp(x - x.max()).sum()
    for name, rg in rgs.items():
        pred, attn, kg_ordered = predict_from_embeddings(m, rg["node_embeddings"], kgd, "cuda")
        ref, _ = orc.forward_list([rg["node_embeddings"].numpy()], kg_real[order][None])
        assert list(kg_ordered) == sorted(names)
        assert_close(pred["mask_logits"].numpy()[0], ref["mask"][0], 2e-5, 1e-5, "mask logits")
        assert_close(pred["mask_prob"].numpy()[0], sm(ref["mask"][0]), 1e-5, 1e-5, "mask prob")
        assert_close(pred["instance_prob"].numpy()[0], sm(ref["instance"][0]), 1e-5, 1e-5, "instance prob")
        assert abs(pred["edge_prob"] - 1 / (1 + np.exp(-float(ref["edge"][0, 0])))) < 1e-5 and abs(pred["score"] - float(ref["score"][0, 0])) < 1e-5
        assert pred["mask_pred"] == int(ref["mask"][0].argmax()) and pred["instance_pred"] == int(ref["instance"][0].argmax())
        assert_close(t2n(attn["rg2kg"][0]), ref["attn_rg2kg"][0], 2e-6, 2e-4, "rg2kg map (columns in sorted-key order)")
    res = predict_embedding_directory(m, rgs, kgd, str(tmp_path / "out"), "cuda", max_images=2)
    with open(tmp_path / "out" / "batch_results.json") as f:
        assert json.load(f) == res
    assert len(res) == 2 and set(res[0]) == {"image", "prediction", "pred_label", "camo_prob", "not_camo_prob", "score"}
    assert res[0]["image"] == "img0.jpg" and res[0]["prediction"] in ("Camouflaged", "Not Camouflaged")
    assert abs(res[0]["camo_prob"] + res[0]["not_camo_prob"] - 1) < 1e-6


def test_tail_kernel_never_times_out_in_this_process():
    """The one-launch tail's bounded waits (three all-reduces among 64 co-resident blocks) must never give up when the
    process has the GPU's CUs to itself; the counter is sticky, so this covers every fused training step the tests above ran."""
    from camouflage_multimodal_amd import _lib
    assert _lib.tail_timeouts() == 0


def test_adamw_leaves_the_next_steps_weight_shadows(kg_real):
    """camo_clip_adamw_shadows: (1) the same parameters, moments and gradients as camo_clip_adamw, bit for bit; (2) the bf16
    weight shadows it leaves are byte-identical to the ones the forward would rebuild from the updated parameters, so a step
    that trusts them (shadows_valid) computes the same thing; (3) a torch-side write to the parameters in between is noticed."""
    import copy
    from camouflage_multimodal_amd import NativeTrainer
    cfg = OP.full_cfg()
    nrs = [303, 64, 33, 530, 17]
    rg = torch.from_numpy(np.concatenate([OP.make_rg(n, 128, seed=50 + i) for i, n in enumerate(nrs)])).cuda()
    kg = torch.from_numpy(np.stack([kg_real] * len(nrs))).cuda()
    y, e, s = (torch.from_numpy(v) for v in OP.make_labels(len(nrs), seed=3))
    ma = make_model(cfg, 1, "bf16").train()
    mb = make_model(cfg, 1, "bf16").train()
    ta, tb = NativeTrainer(ma, reuse_shadows=True), NativeTrainer(mb, reuse_shadows=False)
    # (1) one step each from identical gradients: run the forward/backward once, copy the gradients over
    ea, eb = ma._engine, mb._engine
    ga, gb = ea.ensure_flat_grads(attach=False), eb.ensure_flat_grads(attach=False)
    batch = ea.make_batch(rg, nrs, kg)
    ea.train_raw(batch, ea.workspace(batch), y, e, s, True, 77, ea._gtab, use_shadows=True)
    gb.copy_(ga)
    ta.opt.step(zero_grads=False, shadows=True); tb.opt.step(zero_grads=False, shadows=False)
    torch.cuda.synchronize()
    assert torch.equal(ea.flat_params, eb.flat_params) and torch.equal(ga, gb)
    ma_, va_, _ = ta.opt._state(); mb_, vb_, _ = tb.opt._state()
    assert torch.equal(ma_, mb_) and torch.equal(va_, vb_)
    # (2) the shadows AdamW left == the shadows the forward rebuilds from those parameters
    assert ea.shadows_current()
    left = ea._shadows.clone()
    ea._shadows_version = None                                # force a rebuild into the same buffer
    ea.train_raw(batch, ea.workspace(batch), y, e, s, True, 78, ea._gtab, use_shadows=True)
    torch.cuda.synchronize()
    assert torch.equal(left, ea._shadows)
    # whole steps through the trainer, with and without reuse: the same losses step by step (parameters themselves drift apart by
    # up to lr per step wherever Adam normalises a gradient that is rounding noise -- see helpers.assert_params_close -- so the
    # losses are the robust witness)
    ga.zero_(); gb.zero_()
    mb.load_state_dict(copy.deepcopy(ma.state_dict()))
    tb.opt.load_state_dict(copy.deepcopy(ta.opt.state_dict()))
    for step in range(3):
        la, _ = ta.step(rg, nrs, kg, y, e, s, seed=100 + step); lb, _ = tb.step(rg, nrs, kg, y, e, s, seed=100 + step)
        assert_close(t2n(la), t2n(lb), 1e-4 if step == 0 else 1e-2, 1e-3, f"loss terms, step {step}")
    torch.cuda.synchronize()
    err = np.abs(t2n(ea.flat_params) - t2n(eb.flat_params))
    assert err.max() <= 2.2 * 5e-4 * 3, err.max()
    # (3) staleness: the optimizer just left them current; a load_state_dict makes them stale
    assert ea.shadows_current()
    ma.load_state_dict(copy.deepcopy(mb.state_dict()))
    assert not ea.shadows_current()
    ta.step(rg, nrs, kg, y, e, s, seed=7)                     # rebuilds, then continues
    assert ea.shadows_current()


def test_shadow_reuse_survives_batches_outside_the_fused_schedule(kg_real):
    """The trainer's default (optimizer leaves the weight shadows, next call trusts them) with a batch the fused schedule does
    not take in between (Nk = 17 > 16 runs on the GEMM-per-layer schedule): no error, and the steps after it are the same as
    with reuse switched off (same seeds; fp32-atomics noise only)."""
    from camouflage_multimodal_amd import NativeTrainer
    cfg = OP.full_cfg()
    nrs = [64, 200, 33]
    rg = torch.from_numpy(np.concatenate([OP.make_rg(n, 128, seed=80 + i) for i, n in enumerate(nrs)])).cuda()
    kg13 = torch.from_numpy(np.stack([kg_real] * 3)).cuda()
    kg17 = torch.from_numpy(np.stack([OP.make_kg(17, 128, seed=5 + i) for i in range(3)])).cuda()
    y, e, s = (torch.from_numpy(v) for v in OP.make_labels(3, seed=4))
    res = []
    for reuse in (True, False):
        m = make_model(cfg, 2, "bf16").train()
        tr = NativeTrainer(m, reuse_shadows=reuse)
        losses = []
        for step, kg in enumerate((kg13, kg13, kg17, kg13, kg13)):
            terms, _ = tr.step(rg, nrs, kg, y, e, s, seed=500 + step)
            losses.append(t2n(terms))
        torch.cuda.synchronize()
        assert all(np.isfinite(l).all() for l in losses)
        res.append((losses, t2n(m._engine.flat_params)))
    for step, (la, lb) in enumerate(zip(res[0][0], res[1][0])):           # (parameters drift by Adam's noise; the losses are the witness)
        assert_close(la, lb, 1e-4 if step == 0 else 2e-2, 2e-3, f"loss terms, step {step}")
    assert np.abs(res[0][1] - res[1][1]).max() <= 2.2 * 5e-4 * 5


def test_inference_calls_reuse_the_weight_shadows(kg_real):
    """camo_forward_cached: a validation / prediction loop builds the fused schedule's weight shadows once per parameter change.
    (1) cached and uncached calls give the same outputs; (2) the second call does not touch the shadow buffer; (3) a parameter
    change through torch is noticed and the outputs follow the new parameters; (4) a training step after inference calls
    rebuilds the full set (the inference call leaves the forward set only), and inference right after an optimizer step
    uses what the optimizer left; (5) a batch outside the fused schedule (Nk = 17) leaves the buffer alone and is correct."""
    import copy
    from camouflage_multimodal_amd import NativeTrainer
    cfg = OP.full_cfg()
    nrs = [303, 64, 33, 530, 17]
    rg = torch.from_numpy(np.concatenate([OP.make_rg(n, 128, seed=60 + i) for i, n in enumerate(nrs)])).cuda()
    kg = torch.from_numpy(np.stack([kg_real] * len(nrs))).cuda()
    kg17 = torch.from_numpy(np.stack([OP.make_kg(17, 128, seed=9 + i) for i in range(len(nrs))])).cuda()
    y, e, s = (torch.from_numpy(v) for v in OP.make_labels(len(nrs), seed=5))
    m = make_model(cfg, 3, "bf16").eval()
    tr = NativeTrainer(m)
    eng = m._engine

    def uncached():                       # the plain entry point: shadows rebuilt in the workspace by the call itself
        b = eng.make_batch(rg, nrs, kg)
        outs, _ = eng.forward_raw(b, eng.workspace(b, private=True), False, 0, inference=False)
        return t2n(outs)

    # (1), (2)
    o1 = t2n(tr.evaluate(rg, nrs, kg))
    assert eng.shadows_current() and not eng._shadows_full
    snap = eng._shadows.clone()
    eng._shadows[-4096:].fill_(0x5A)      # the transposed set's tail is not part of the forward set: an inference call must not need it
    o2 = t2n(tr.evaluate(rg, nrs, kg))
    torch.cuda.synchronize()
    assert torch.equal(eng._shadows[:-4096], snap[:-4096])
    ref = uncached()
    assert_close(o1, ref, 2e-6, 1e-5, "cached (building) call vs plain call")
    assert_close(o2, ref, 2e-6, 1e-5, "cached (reusing) call vs plain call")
    # (3)
    other = make_model(cfg, 4, "bf16")
    m.load_state_dict(copy.deepcopy(other.state_dict()))
    assert not eng.shadows_current()
    o3 = t2n(tr.evaluate(rg, nrs, kg))
    assert eng.shadows_current()
    assert_close(o3, uncached(), 2e-6, 1e-5, "after load_state_dict")
    assert np.abs(o3 - o1).max() > 1e-3
    # (5)
    before = eng._shadows.clone()
    o17 = t2n(tr.evaluate(rg, nrs, kg17))
    b17 = eng.make_batch(rg, nrs, kg17)
    p17, _ = eng.forward_raw(b17, eng.workspace(b17, private=True), False, 0, inference=False)
    assert_close(o17, t2n(p17), 2e-6, 1e-5, "Nk = 17")
    assert torch.equal(before, eng._shadows) and eng.shadows_current()
    # (4) training after inference: same losses as a trainer that never reuses anything
    m2 = make_model(cfg, 4, "bf16").train(); m.train()
    t2 = NativeTrainer(m2, reuse_shadows=False)
    for step in range(3):
        la, _ = tr.step(rg, nrs, kg, y, e, s, seed=900 + step); lb, _ = t2.step(rg, nrs, kg, y, e, s, seed=900 + step)
        assert_close(t2n(la), t2n(lb), 1e-4 if step == 0 else 1e-2, 1e-3, f"loss terms, step {step}")
        if step == 1:                     # a validation pass in the middle of training: uses the optimizer's shadows, leaves them usable
            m.eval(); m2.eval()
            assert eng.shadows_current() and eng._shadows_full
            va = t2n(tr.evaluate(rg, nrs, kg)); vb = t2n(t2.evaluate(rg, nrs, kg))
            assert eng.shadows_current() and eng._shadows_full
            assert_close(va, vb, 5e-3, 5e-3, "validation outputs in the middle of training")
            m.train(); m2.train()


def test_tail_timeout_is_not_applied(kg_real):
    """A one-launch tail whose arrival wait gives up (co-residency lost: GPU shared with another process) must not become a
    parameter update.  The developer hook makes one block skip its arrival, so the other 63 time out deterministically: the
    step's loss terms are NaN, the gradient norm is NaN, parameters and Adam moments are untouched, the sticky counter moved;
    the next step is a normal one."""
    from camouflage_multimodal_amd import NativeTrainer, _lib
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").train()
    tr = NativeTrainer(m)
    nrs = [40, 33, 70, 12]
    rg = torch.from_numpy(np.concatenate([OP.make_rg(n, 128, seed=40 + i) for i, n in enumerate(nrs)])).cuda()
    kg = torch.from_numpy(np.stack([kg_real] * 4)).cuda()
    y, e, s = (torch.from_numpy(x) for x in OP.make_labels(4, seed=3))
    tr.step(rg, nrs, kg, y, e, s)                                    # a normal step first (Adam moments non-zero)
    torch.cuda.synchronize()
    before = m._engine.flat_params.clone()
    t0 = _lib.tail_timeouts()
    m._engine.set_option("tail_skip_arrival", 6)                     # (one shot, this engine's next call)
    terms, _ = tr.step(rg, nrs, kg, y, e, s)
    torch.cuda.synchronize()
    assert _lib.tail_timeouts() > t0
    assert m._engine.options.tail_skip_arrival == 0                  # (the step's tail launch took the hook)
    assert torch.isnan(terms).all()
    assert not np.isfinite(t2n(tr.opt.grad_norm())[0])
    assert torch.equal(m._engine.flat_params, before), "a timed-out step changed the parameters"
    terms, _ = tr.step(rg, nrs, kg, y, e, s)                         # and the next step is applied again
    torch.cuda.synchronize()
    assert torch.isfinite(terms).all() and not torch.equal(m._engine.flat_params, before)
    assert torch.isfinite(m._engine.flat_params).all()


def test_train_multimodal_fixed_end_to_end_on_disk(tmp_path, kg_real):
    """The reference's training driver (train_multimodal.py:347-492) from files on disk: an RG embedding dict and a KG embedding
    dict saved with torch.save (the reference's .pt formats), three directories of ground-truth PNGs, the YAML's keys -- two
    epochs through EmbeddingMatcher -> SmartMultimodalDataset -> 80/20 split -> weighted sampling -> device-resident minibatches
    (a fresh Nr tuple per step) -> NativeTrainer, then the checkpoint it wrote loads into the inference path."""
    from PIL import Image
    from camouflage_multimodal_amd import load_multimodal_model, train_multimodal_fixed
    names = [str(n) for n in load_golden("kg_embeddings")["names"]]
    torch.save({n: torch.from_numpy(kg_real[i:i + 1].copy()) for i, n in enumerate(names)}, tmp_path / "kg.pt")
    rs = np.random.RandomState(5)
    rg, dirs = {}, {k: tmp_path / k for k in ("gt_object", "gt_instance", "gt_edge")}
    for d in dirs.values():
        d.mkdir()
    for i in range(30):
        name = f"COD10K-CAM-1-Aquatic-{i}-{'Fish' if i % 2 else 'Bird'}-{i}"
        n = int(rs.randint(20, 90))
        rg[name + ".jpg"] = {"node_embeddings": torch.from_numpy(OP.make_rg(n, 128, seed=700 + i)), "graph_embedding": torch.zeros(1, 128), "num_nodes": n}
        m = np.zeros((64, 80), np.uint8)
        if i % 3:                                                            # two thirds camouflaged (a blob), one third empty
            m[8:8 + 30 + i % 7, 10:60] = 255
        for k in ("gt_object", "gt_instance"):
            Image.fromarray(m, mode="L").save(dirs[k] / f"{name}.png")
        Image.fromarray(np.full((64, 80), 30 if i % 2 else 0, np.uint8), mode="L").save(dirs["gt_edge"] / f"{name}.png")
    torch.save(rg, tmp_path / "rg.pt")
    ck = tmp_path / "ckpt"
    cfg = {"rg_embeddings_path": str(tmp_path / "rg.pt"), "kg_embeddings_path": str(tmp_path / "kg.pt"), "use_all_kg_categories": True,
           "mask_dir": str(dirs["gt_object"]), "instance_dir": str(dirs["gt_instance"]), "edge_dir": str(dirs["gt_edge"]),
           "model": dict(rg_dim=128, kg_dim=128, hidden_dim=256, num_heads=8, fusion_type="cross_attention", num_classes=2, dropout=0.3),
           "epochs": 2, "batch_size": 4, "learning_rate": 5e-4, "weight_decay": 1e-4, "checkpoint_dir": str(ck), "precision": "bf16"}
    logs = []
    model, hist = train_multimodal_fixed(cfg, device="cuda", seed=1, log=logs.append)
    assert len(hist["train_loss"]) == 2 and all(np.isfinite(v) for k in hist for v in hist[k])
    assert "Train: 24 | Val: 6" in logs[0]
    with open(ck / "training_history_fixed.json") as f:
        assert json.load(f) == hist
    if os.path.exists(ck / "multimodal_best_fixed.pth"):                       # (written when an epoch's validation F1 of class 1 is > 0)
        m2, c2 = load_multimodal_model(str(ck / "multimodal_best_fixed.pth"), device="cuda")
        assert set(model.state_dict()) == set(m2.state_dict()) and c2["model"] == cfg["model"]


def test_gather_batch_kernel_matches_index_ops_and_augments_in_distribution():
    """camo_gather_batch (one launch: packed rows, KG rows, labels, packed offsets, augmentation) against torch index ops on the
    same device-resident dataset; the augmentation's statistics: about half the samples get noise, N(0, 0.01^2), on both streams."""
    from camouflage_multimodal_amd import DeviceResidentDataset
    rs = np.random.RandomState(2)
    nrs_all = [int(x) for x in rs.randint(1, 200, size=300)]
    samples = [dict(rg_node_emb=torch.from_numpy(rs.standard_normal((n, 128)).astype(np.float32)), kg_emb=torch.from_numpy(rs.standard_normal((13, 1, 128)).astype(np.float32)),
                    mask_label=i % 2, edge_label=float(i % 3 == 0), score_label=0.01 * i) for i, n in enumerate(nrs_all)]
    ds = DeviceResidentDataset(samples, "cuda")
    for idx in ([5], [299, 0, 0, 17, 123, 7], [int(x) for x in rs.randint(0, 300, size=257)]):
        rg, nrs, kg, y, e, s = ds.batch(idx)
        torch.cuda.synchronize()
        assert list(nrs) == [nrs_all[i] for i in idx]
        assert nrs.offsets_dev.cpu().tolist() == [0] + list(np.cumsum(nrs))
        assert torch.equal(rg.cpu(), torch.cat([samples[i]["rg_node_emb"] for i in idx]))
        assert torch.equal(kg.cpu(), torch.stack([samples[i]["kg_emb"].reshape(13, 128) for i in idx]))
        assert y.cpu().tolist() == [i % 2 for i in idx] and torch.equal(s.cpu(), torch.tensor([0.01 * i for i in idx], dtype=torch.float32))
        dev_idx = torch.tensor(idx, device="cuda")
        rg2, nrs2, *_ = ds.batch(idx, idx_dev=dev_idx)                          # indices handed over as a device tensor
        assert torch.equal(rg, rg2) and list(nrs2) == list(nrs)
    aug = DeviceResidentDataset(samples, "cuda", augment=True, seed=3)
    idx = list(range(300))
    rg, nrs, kg, *_ = aug.batch(idx)
    d = (rg.cpu() - torch.cat([s_["rg_node_emb"] for s_ in samples])).numpy()
    off = np.concatenate([[0], np.cumsum(nrs)])
    noisy = np.array([np.abs(d[off[i]:off[i + 1]]).max() > 0 for i in range(300)])
    assert 0.35 < noisy.mean() < 0.65                                        # a fair coin per sample
    dk = (kg.cpu() - torch.stack([s_["kg_emb"].reshape(13, 128) for s_ in samples])).numpy()
    assert np.array_equal(noisy, np.abs(dk).reshape(300, -1).max(1) > 0)     # the same coin for both streams
    z = np.concatenate([d[off[i]:off[i + 1]].ravel() for i in range(300) if noisy[i]])
    assert abs(z.mean()) < 2e-4 and abs(z.std() - 0.01) < 3e-4 and abs((np.abs(z) < 0.01).mean() - 0.6827) < 0.01
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 0.01
    rg_b, *_ = aug.batch(idx)                                                # a second draw: other noise
    assert not torch.equal(rg, rg_b)


@pytest.mark.parametrize("B,lo,hi", [(1, 5, 6), (17, 1, 200), (300, 1, 90), (1000, 1, 70), (64, 300, 531)])
def test_batch_descriptor_tables(B, lo, hi):
    """camo_prepare_batch (misc.hip, batchdesc_kernel: one launch) against a host restatement of the tables it builds: row -> sample,
    1 / Nr, the first 32-row tile of every sample and the per-tile {sample, first packed row, rows, 1 / Nr} entries; -1 marks the unused
    tail of the tile table.  B > 256 takes the several-samples-per-thread scan."""
    import ctypes as C
    from camouflage_multimodal_amd import _lib
    rs = np.random.RandomState(B)
    nrs = rs.randint(lo, hi, size=B).astype(np.int64)
    offs = np.zeros(B + 1, np.int32); offs[1:] = np.cumsum(nrs)
    T = int(offs[-1])
    L = _lib.lib()
    nbytes = L.camo_batch_desc_bytes(B, T)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    offs_d = torch.from_numpy(offs).cuda()
    _lib.check(L.camo_prepare_batch(C.c_void_p(offs_d.data_ptr()), B, T, int(nrs.max()), C.c_void_p(buf.data_ptr()), nbytes,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "camo_prepare_batch")
    raw = buf.cpu().numpy()
    al = lambda x: (x + 255) & ~255
    o = 0
    row_sample = raw[o:o + 4 * T].view(np.int32); o = al(o + 4 * T)
    inv_nr = raw[o:o + 4 * B].view(np.float32); o = al(o + 4 * B)
    tile_off = raw[o:o + 4 * (B + 1)].view(np.int32); o = al(o + 4 * (B + 1))
    ntab = T // 32 + B
    tile_desc = raw[o:o + 16 * ntab].view(np.int32).reshape(ntab, 4)
    assert np.array_equal(row_sample, np.repeat(np.arange(B), nrs))
    assert np.array_equal(inv_nr, (1.0 / nrs.astype(np.float32)).astype(np.float32))
    tiles = (nrs + 31) // 32
    want_off = np.zeros(B + 1, np.int64); want_off[1:] = np.cumsum(tiles)
    assert np.array_equal(tile_off, want_off)
    want = np.full((ntab, 4), 0, np.int32); want[:, 0] = -1
    k = 0
    for b in range(B):
        for j in range(int(tiles[b])):
            r0 = int(offs[b]) + 32 * j
            want[k] = (b, r0, min(32, int(offs[b + 1]) - r0), np.float32(1.0 / np.float32(nrs[b])).view(np.int32))
            k += 1
    assert np.array_equal(tile_desc[:k], want[:k])
    assert (tile_desc[k:, 0] == -1).all()


def test_writers_torch_cannot_see_need_invalidate_shadows(kg_real):
    """A write through ``flat_params.data`` (what an in-place collective such as a parameter broadcast amounts to) bumps no
    version counter: the engine keeps believing its bf16 weight shadows.  ``invalidate_shadows()`` is the contract for such
    writers (``ddp.broadcast_parameters`` calls it): after it the next call rebuilds the shadows and follows the new weights."""
    from camouflage_multimodal_amd import NativeTrainer
    cfg = OP.full_cfg()
    nrs = [200, 77, 31]
    rg = torch.from_numpy(np.concatenate([OP.make_rg(n, 128, seed=80 + i) for i, n in enumerate(nrs)])).cuda()
    kg = torch.from_numpy(np.stack([kg_real] * len(nrs))).cuda()
    m = make_model(cfg, 3, "bf16").eval()
    other = make_model(cfg, 4, "bf16").eval()
    tr = NativeTrainer(m)
    eng = m._engine
    o_old = t2n(tr.evaluate(rg, nrs, kg))
    assert eng.shadows_current()
    eng.flat_params.data.copy_(other._engine.flat_params.data)        # invisible to torch's version counters
    assert eng.shadows_current()                                      # ... and so to the engine: the stale shadows would be used
    eng.invalidate_shadows()
    assert not eng.shadows_current()
    o_new = t2n(tr.evaluate(rg, nrs, kg))
    want = t2n(NativeTrainer(other).evaluate(rg, nrs, kg))
    assert_close(o_new, want, 2e-6, 1e-5, "after invalidate_shadows the call follows the new parameters")
    assert float(np.abs(o_new - o_old).max()) > 1e-3
