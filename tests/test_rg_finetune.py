"""The region-graph fine-tuner (camouflage_multimodal_amd/rg_finetune.py): prepare_finetune_batch and
RegionGraphFineTuner against the parts they are made of and against a float64 trajectory.

The tuner adds no arithmetic of its own: a step is camo_rg_loss_backward (tests/test_rg_train.py) into a flat buffer and
camo_grad_sumsq + camo_clip_adamw (tests/test_hip_optimizer.py) over flat buffers.  So the first GPU test asks for the BYTES those
parts leave when they are called one by one on copies.  The second runs three steps beside torch: tests/rg_train_ref.py forward and
loss, autograd, clip_grad_norm_, torch.optim.AdamW, all in float64, and holds the losses of every step and the parameter updates
p3 - p0 to the convention of tests/test_rg_train.py,

    e = max|d - d64| / max(max|d64|, 1e-12)  <=  8 e32 + 2e-6,

e32 being the error of the same trajectory in torch-CPU float32, computed in the same test.  The reference asserts at every step that
no pre-activation lies within FLIP_MARGIN of 0: the case is "batch" of tests/test_rg_train.py (margin 2.3e-4 at its start), and at
LR = 2e-6 the three AdamW steps move the nearest pre-activation by a tenth of that (margins 2.3e-4, 2.4e-4, 2.1e-4 on the CPU; at 1e-5
one of them crosses 0 during the third step).  An update of 6e-6 on a batch-norm weight near 1 is a hundred float32 ulps, so e32 of
the updates is about 3e-2 there: what fp32 parameters cost, measured rather than assumed.  On an MI355X e equals e32 to three digits
for 30 of the 32 parameters, and the largest e / e32 was 1.79 and 1.32 in two runs (conv1.att_dst).
"""
import numpy as np
import pytest
import torch

import rg_targets_ref as TG
import rg_train_ref as TR
from oracle import rg_gnn_oracle as RO
from test_rg_train import NAMES, _bits, _case, _csr_pair, _data, _err, _model, _targets

LR, WD, BETAS, EPS, MAX_NORM = 2e-6, 1e-2, (0.9, 0.999), 1e-8, 0.25      # (the gradient norm of "batch" is 0.35: the clip is active)
HYPER = dict(lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, max_norm=MAX_NORM)


def _shapes():
    from camouflage_multimodal_amd import RegionGraphGNN
    return [tuple(p.shape) for p in RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).trainable_parameters()]


def _trajectory(p, x, ei, ew, mt, it, et, heads, nc, steps, dtype, lr, weight_decay, betas, eps, max_norm):
    """`steps` steps of clip_grad_norm_ + torch.optim.AdamW on the restatement's loss in `dtype` -> (losses [steps][4] of the
    parameters before each step, flip margin before each step, pre-clip gradient norms, {name: p_steps - p_0 as float64})."""
    n = x.shape[0]
    src, dst, w = RO.with_self_loops(n, ei, ew)
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in p.items()}
    params = [P[k].requires_grad_(True) for k in NAMES]
    start = {k: P[k].detach().clone() for k in NAMES}
    opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    xt, src, dst, w = torch.tensor(x, dtype=dtype), torch.tensor(src), torch.tensor(dst), torch.tensor(w, dtype=dtype)
    mt, it, et = torch.tensor(mt, dtype=torch.int64), torch.tensor(it, dtype=torch.int64), torch.tensor(et, dtype=dtype)
    losses, margins, norms = [], [], []
    for _ in range(steps):
        taps = []
        ls = TR.losses(TR.forward(P, xt, src, dst, w, heads, taps), mt, it, et, (1.0, 1.0, 1.0), nc)
        opt.zero_grad()
        ls[0].backward()
        margins.append(min(float(t.abs().min() / t.abs().max()) for t in taps if t.numel()))
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
        losses.append([float(v.detach()) for v in ls])
    return losses, margins, norms, {k: (P[k].detach() - start[k]).double().numpy() for k in NAMES}


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_flat_layout_is_the_gradient_layout():
    from camouflage_multimodal_amd.rg_finetune import flat_layout
    shapes = _shapes()
    pieces, total = flat_layout(shapes)
    assert len(pieces) == 32 and total % 64 == 0
    at = 0
    for (o, n), shape in zip(pieces, shapes):
        assert o == at and o % 64 == 0 and n == int(np.prod(shape))
        at += -(-n // 64) * 64                                         # what loss_and_gradients_csr gives its gradients
    assert at == total


def test_tuner_on_cpu_tensors_keeps_the_model_and_its_state_dict():
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN
    c = _case("batch")
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    tuner = RegionGraphFineTuner(m, **HYPER)
    named = {id(p): k for k, p in m.named_parameters()}
    assert [named[id(e[0])] for e in tuner._layout()] == NAMES == [e[1] for e in tuner._layout()]
    flat = tuner.flat_params
    used = torch.zeros(flat.numel(), dtype=torch.bool)
    for p, (q, name, o, n, shape) in zip(m.trainable_parameters(), tuner._layout()):
        assert q is p and o % 64 == 0 and p.data_ptr() == flat.data_ptr() + 4 * o and tuple(p.shape) == shape and p.is_contiguous(), name
        used[o:o + n] = True
    assert bool((flat[~used] == 0).all()) and int((~used).sum()) > 0
    for k, v in m.state_dict().items():                               # nothing changed value, running statistics included
        assert torch.equal(v, before[k]), k
    sd = m.state_dict()                                               # load_state_dict writes through the views
    for k, v in c["p"].items():
        sd[k] = torch.from_numpy(v.copy())
    m.load_state_dict(sd, strict=True)
    tuner._check_resident()
    for p, (q, name, o, n, shape) in zip(m.trainable_parameters(), tuner._layout()):
        assert np.array_equal(flat[o:o + n].numpy(), c["p"][name].reshape(-1)), name
    assert bool((flat[~used] == 0).all())
    again = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2)
    again.load_state_dict(m.state_dict(), strict=True)
    for k, v in again.state_dict().items():
        assert torch.equal(v, m.state_dict()[k]), k
    # the optimizer state has torch.optim.AdamW's shape and goes round
    tuner.step_count = 3
    tuner._m.uniform_(-1, 1)
    tuner._v.uniform_(0, 1)
    osd = tuner.state_dict()
    ref = torch.optim.AdamW(m.trainable_parameters(), lr=LR).state_dict()
    assert set(osd) == set(ref) and set(ref["param_groups"][0]) <= set(osd["param_groups"][0]) and osd["param_groups"][0]["params"] == list(range(32))
    other = RegionGraphFineTuner(RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2))
    other.load_state_dict(osd)
    assert other.step_count == 3 and other.lr == LR and other.weight_decay == WD
    for (_, name, o, n, _s) in tuner._layout():
        assert torch.equal(other._m[o:o + n], tuner._m[o:o + n]) and torch.equal(other._v[o:o + n], tuner._v[o:o + n]), name
    assert tuner.set_epoch(5) < LR and tuner.set_epoch(0) == LR


def test_the_reference_trajectory_stays_clear_of_a_relu_flip():
    c = _case("batch")
    losses, margins, norms, _ = _trajectory(c["p"], c["x"], c["ei"], c["ew"], c["mt"], c["it"], c["et"], c["heads"], c["nc"], 3, torch.float64, **HYPER)
    print("margins", margins, "gradient norms", norms)
    assert min(margins) > TR.FLIP_MARGIN and min(norms) > MAX_NORM
    assert losses[2][0] < losses[1][0] < losses[0][0]


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _batch(c, d):
    from camouflage_multimodal_amd.rg_finetune import FineTuneBatch
    csr, rcsr = _csr_pair(c, d)
    mt, it, et = _targets(c)
    return FineTuneBatch(d, None, None, mt, it, et, None, csr, rcsr)


def _padding(tuner):
    used = torch.zeros(tuner.flat_params.numel(), dtype=torch.bool, device=tuner.flat_params.device)
    for _, _, o, n, _ in tuner._layout():
        used[o:o + n] = True
    return ~used


@pytest.mark.gpu
def test_one_step_is_its_parts():
    """Steps 1 to 3 through the tuner leave, bit for bit, what loss_and_gradients_csr on the same CSR pair, a copy of its gradients into a
    flat buffer, camo_grad_sumsq and camo_clip_adamw leave when called one by one on copies; compared after step 1 and after step 3."""
    from camouflage_multimodal_amd import RegionGraphFineTuner, _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    c = _case("batch")
    m, d = _model(c).eval(), _data(c)
    batch = _batch(c, d)
    tuner = RegionGraphFineTuner(m, **HYPER)
    shadow = _model(c).eval()                                          # the parts run on a model of its own, parameters wherever torch put them
    lay = tuner._layout()
    p = tuner.flat_params.clone()
    g, mm, vv = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    ss = torch.zeros(_lib.SUMSQ_FLOATS, dtype=torch.float32, device="cuda")
    L = _lib.lib()
    for step in (1, 2, 3):
        got = tuner.step(batch)
        assert set(got) == {"loss", "mask_loss", "instance_loss", "edge_loss"} and all(v.dim() == 0 and v.is_cuda for v in got.values())
        loss, grads = shadow.loss_and_gradients_csr(d.x, batch.csr, batch.reversed_csr, batch.mask_target, batch.instance_target, batch.edge_target)
        for (_, name, o, n, shape), gr in zip(lay, grads):
            g[o:o + n].copy_(gr.reshape(-1))
        _lib.check(L.camo_grad_sumsq(_ptr(g), g.numel(), _ptr(ss), _stream_ptr()), "camo_grad_sumsq")
        _lib.check(L.camo_clip_adamw(_ptr(p), _ptr(g), _ptr(mm), _ptr(vv), g.numel(), _ptr(ss), MAX_NORM, LR, BETAS[0], BETAS[1], EPS, WD, step, 0,
                                     _stream_ptr()), "camo_clip_adamw")
        with torch.no_grad():
            for q, (_, name, o, n, shape) in zip(shadow.trainable_parameters(), lay):
                q.copy_(p[o:o + n].view(shape))
        if step == 2:
            continue
        for i, k in enumerate(("loss", "mask_loss", "instance_loss", "edge_loss")):
            assert np.array_equal(_bits(got[k].cpu()), _bits(loss[i].cpu())), (step, k)
        for name, a, b in (("p", tuner.flat_params, p), ("m", tuner._m, mm), ("v", tuner._v, vv), ("g", tuner.flat_grads, g)):
            assert np.array_equal(_bits(a.cpu()), _bits(b.cpu())), (step, name)
        assert np.array_equal(_bits(tuner.grad_norm().cpu()), _bits(ss[:1].sqrt().cpu()))
    assert tuner.step_count == 3 and not torch.equal(tuner.flat_params, torch.zeros_like(p)) and bool((tuner._v > 0).any())
    for q, (r, name, o, n, shape) in zip(shadow.trainable_parameters(), lay):      # the model's own parameters ARE the flat buffer
        assert torch.equal(r.data, q.data), name


@pytest.mark.gpu
def test_three_steps_follow_the_float64_trajectory():
    c = _case("batch")
    args = (c["p"], c["x"], c["ei"], c["ew"], c["mt"], c["it"], c["et"], c["heads"], c["nc"], 3)
    l64, margins, norms, d64 = _trajectory(*args, torch.float64, **HYPER)
    assert min(margins) > TR.FLIP_MARGIN, margins                       # on the CPU reference, at every step
    l32, _, _, d32 = _trajectory(*args, torch.float32, **HYPER)
    from camouflage_multimodal_amd import RegionGraphFineTuner
    m, d = _model(c).eval(), _data(c)
    start = {k: p.detach().cpu().numpy().astype(np.float64) for k, p in zip(NAMES, m.trainable_parameters())}
    tuner = RegionGraphFineTuner(m, **HYPER)
    batch = _batch(c, d)
    got = [tuner.step(batch) for _ in range(3)]
    worst = 0.0
    for s in range(3):
        for i, k in enumerate(("loss", "mask_loss", "instance_loss", "edge_loss")):
            e, e32 = _err(float(got[s][k]), l64[s][i]), _err(l32[s][i], l64[s][i])
            print(f"step {s + 1} {k}: e {e:.3g} e32 {e32:.3g}")
            worst = max(worst, e / e32) if e32 > 0 else worst
            assert e <= 8 * e32 + 2e-6, (s, k, e, e32)
    for k, p in zip(NAMES, m.trainable_parameters()):
        upd = p.detach().cpu().numpy().astype(np.float64) - start[k]
        e, e32 = _err(upd, d64[k]), _err(d32[k], d64[k])
        print(f"update {k}: e {e:.3g} e32 {e32:.3g}")
        worst = max(worst, e / e32) if e32 > 0 else worst
        assert np.abs(d64[k]).max() > 0 and e <= 8 * e32 + 2e-6, (k, e, e32)
    print(f"largest e / e32: {worst:.3g}")


@pytest.mark.gpu
def test_five_steps_leave_the_running_statistics_and_the_padding_alone():
    from camouflage_multimodal_amd import RegionGraphFineTuner, _lib
    c = _case("batch")
    m, d = _model(c).train(), _data(c)                                 # (whatever the mode)
    stats = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    assert len(stats) == 12
    tuner = RegionGraphFineTuner(m, lr=1e-3)
    batch, pad = _batch(c, d), _padding(tuner)
    before = tuner.flat_params.clone()
    for _ in range(5):
        tuner.step(batch)
    for k, v in m.state_dict().items():
        if k in stats:
            assert v.data_ptr() != 0 and np.array_equal(v.cpu().numpy().reshape(-1).view(np.uint8), stats[k].cpu().numpy().reshape(-1).view(np.uint8)), k
    for name, buf in (("p", tuner.flat_params), ("g", tuner.flat_grads), ("m", tuner._m), ("v", tuner._v)):
        assert bool((buf[pad] == 0).all()), name
    assert bool((tuner.flat_params[~pad] != before[~pad]).any()) and bool(torch.isfinite(tuner.flat_params).all())
    m.to("cpu")
    with pytest.raises(_lib.CamoError, match="RegionGraphFineTuner"):
        tuner.step(batch)


def _rectangle_images():
    rs = np.random.RandomState(21)
    yy, xx = np.mgrid[0:70, 0:33]
    img = np.empty((2, 70, 33, 3), np.float32)
    gt = np.zeros((2, 70, 33), np.uint8)
    for i, (y0, y1, x0, x1) in enumerate(((12, 40, 6, 22), (30, 62, 10, 30))):
        ground = 0.25 + 0.1 * np.sin(yy / 3.0 + i) * np.cos(xx / 2.5) + rs.uniform(-0.04, 0.04, (70, 33))
        img[i] = np.stack([ground, ground * 0.9 + 0.02, ground * 0.8 + 0.05], -1)
        img[i, y0:y1, x0:x1] += 0.5
        gt[i, y0:y1, x0:x1] = 255
    return np.clip(img, 0, 1), gt


@pytest.mark.gpu
def test_from_images_the_targets_are_the_references_and_twenty_steps_learn():
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN, prepare_finetune_batch, segmentation_metrics
    img, gt = _rectangle_images()
    batch = prepare_finetune_batch(torch.from_numpy(img).cuda(), torch.from_numpy(gt).cuda(), n_segments=30)
    seg, rmap, off = batch.segments.cpu().numpy(), batch.region_map.cpu().numpy(), batch.graphs.node_offsets
    want = TG.node_targets(seg, rmap, off, gt)
    got = [t.cpu().numpy() for t in (batch.mask_target, batch.instance_target, batch.edge_target, batch.counts)]
    for name, g, w in zip(("mask_t", "inst_t", "edge_t", "counts"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    n = off[2]
    assert n == batch.graphs.x.shape[0] and {0, 1} <= set(want[0].tolist()) and {0.0, 1.0} <= set(want[2].tolist())
    assert batch.csr[0].shape[0] == n + 1 and batch.reversed_csr[1].shape[0] == batch.csr[1].shape[0] == batch.graphs.edge_index.shape[1] + n
    # the float64 trajectory on the graph and targets the device built: it must learn with room to spare
    lr, steps = 1e-2, 20
    torch.manual_seed(3)
    model = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2)
    p = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if "num_batches" not in k}
    hyper = dict(lr=lr, weight_decay=WD, betas=BETAS, eps=EPS, max_norm=1.0)
    ref, _, _, _ = _trajectory(p, batch.graphs.x.cpu().numpy(), batch.graphs.edge_index.cpu().numpy(), batch.graphs.edge_attr.reshape(-1).cpu().numpy(),
                               want[0], want[1], want[2], 2, 2, steps, torch.float64, **hyper)
    print("reference loss", ref[0][0], "->", ref[-1][0])
    assert ref[-1][0] <= 0.9 * ref[0][0]
    tuner = RegionGraphFineTuner(model.cuda(), **hyper)
    losses = torch.stack([tuner.step(batch)["loss"] for _ in range(steps)]).cpu().numpy()
    print("device loss", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    metrics = tuner.evaluate(torch.from_numpy(img).cuda(), torch.from_numpy(gt).cuda(), n_segments=30)
    assert len(metrics) == 2 and all(set(r) == set(segmentation_metrics([[1, 1, 1, 1, 0]], 2, 2)[0]) for r in metrics)
    again = tuner.step_from_images(torch.from_numpy(img).cuda(), torch.from_numpy(gt).cuda(), n_segments=30)
    assert again["loss"].dim() == 0 and again["loss"].is_cuda and np.isfinite(float(again["loss"])) and tuner.step_count == steps + 1
