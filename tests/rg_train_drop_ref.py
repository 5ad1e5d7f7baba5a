"""torch restatement of include/camo_rg_train_drop.h -- TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED (the reference tree, torch_geometric
and an RG checkpoint are absent): the header's text is the definition.  This file says the forward of tests/rg_train_ref.py (batch norm
frozen) or of tests/rg_train_bn_ref.py (batch statistics) again with inverted dropout at the header's eight sites.  The masks are
oracle.fusion_oracle.dropout_keep on the header's element indices, the multiplier is the fp32 1 / (1 - p) promoted, the loss is
rg_train_ref's and the gradients are autograd's.  tests/test_rg_train_drop.py ties it at rate 0 to both older restatements and holds the
HIP kernels to its gradients."""
import numpy as np
import torch

from oracle import rg_gnn_oracle as RO
from oracle.fusion_oracle import dropout_keep

import rg_detect_ref as R
import rg_train_bn_ref as BR
from rg_train_ref import EPS, FLIP_MARGIN, losses, trainable_names  # noqa: F401

SITE_CONV0, SITE_SHARED, SITE_HEADS = 32, 36, 37            # CAMO_RGT_SITE_* (a CPU test holds them to the header)


def rate32(p):
    """The rate as the C ABI receives it."""
    return float(np.float32(p))


def keep_mask(seed, site, rows, cols, p):
    """Boolean [rows, cols]: dropout_keep on the element indices r * cols + c."""
    idx = np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols)
    return dropout_keep(int(seed), site, idx, np.float32(p))


def multiplier(p):
    """fp32 1 / (1 - p), as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def drop(t, seed, site, p, masks=None):
    """t [rows, cols] through the site's dropout (identity at p == 0).  `masks`: a dict that receives site -> boolean mask."""
    if not p > 0.0:
        return t
    keep = keep_mask(seed, site, t.shape[0], t.shape[1], p)
    if masks is not None:
        masks[site] = keep
    return t * (torch.from_numpy(keep).to(t.dtype) * multiplier(p))


def forward(P, x, src, dst, w, heads, rates=(0.0, 0.0, 0.0), seed=0, batch=False, taps=None, momentum=BR.MOMENTUM, stats=None, masks=None):
    """logits [n, 2 c + 1].  batch False: rg_train_ref.forward's batch norm (running statistics); True: rg_train_bn_ref.forward's (the
    call's own nodes; `stats` as there).  `taps`: the nine pre-activations of the older restatements, in their order."""
    pc, ps, ph = (rate32(v) for v in rates)
    n, hidden = x.shape[0], P["conv1.bias"].shape[0]
    tap = (lambda t: taps.append(t.detach())) if taps is not None else (lambda t: None)
    st = {"mu": [], "var": [], "running": {}}

    def bn(v, k):
        if not batch:
            return (v - P[f"bn{k}.running_mean"]) / torch.sqrt(P[f"bn{k}.running_var"] + EPS) * P[f"bn{k}.weight"] + P[f"bn{k}.bias"]
        y, mu, var, rm, rv = BR.bn_step(v, P[f"bn{k}.weight"], P[f"bn{k}.bias"], P[f"bn{k}.running_mean"], P[f"bn{k}.running_var"], momentum)
        st["mu"].append(mu); st["var"].append(var)
        st["running"][f"bn{k}.running_mean"], st["running"][f"bn{k}.running_var"] = rm, rv
        return y

    h = (x @ P["conv1.lin.weight"].T).reshape(n, heads, hidden)
    a_src = (h * P["conv1.att_src"].reshape(1, heads, hidden)).sum(-1)
    a_dst = (h * P["conv1.att_dst"].reshape(1, heads, hidden)).sum(-1)
    s = a_src[src] + a_dst[dst]
    tap(s)
    e = torch.nn.functional.leaky_relu(s, 0.2)
    idx = dst[:, None].expand(-1, heads)
    m = torch.full((n, heads), -float("inf"), dtype=x.dtype).scatter_reduce(0, idx, e.detach(), "amax")      # (a shift: no gradient)
    p = torch.exp(e - m[dst])
    alpha = p / torch.zeros(n, heads, dtype=x.dtype).index_add(0, dst, p)[dst]
    out = torch.zeros(n, heads, hidden, dtype=x.dtype).index_add(0, dst, alpha[:, :, None] * h[src])
    y = bn(out.mean(1) + P["conv1.bias"], 1)
    tap(y)
    h = drop(torch.relu(y), seed, SITE_CONV0, pc, masks)
    deg = torch.zeros(n, dtype=x.dtype).index_add(0, dst, w)
    dinv = torch.where(deg > 0, deg.clamp_min(1e-30).rsqrt(), torch.zeros_like(deg))
    norm = dinv[src] * w * dinv[dst]
    for k in (2, 3, 4):
        xw = h @ P[f"conv{k}.lin.weight"].T
        y = bn(torch.zeros_like(xw).index_add(0, dst, norm[:, None] * xw[src]) + P[f"conv{k}.bias"], k)
        tap(y)
        h = drop(torch.relu(y), seed, SITE_CONV0 + k - 1, pc, masks)
    y = h @ P["fc_shared.weight"].T + P["fc_shared.bias"]
    tap(y)
    emb = drop(torch.relu(y), seed, SITE_SHARED, ps, masks)
    zs = []
    for name in R.HEADS:
        y = emb @ P[f"{name}_1.weight"].T + P[f"{name}_1.bias"]
        tap(y)
        zs.append(torch.relu(y))
    Z = drop(torch.cat(zs, 1), seed, SITE_HEADS, ph, masks)            # the concatenated [n, 3 hidden / 2]: one index space
    hh = hidden // 2
    cols = [Z[:, i * hh:(i + 1) * hh] @ P[f"{name}_2.weight"].T + P[f"{name}_2.bias"] for i, name in enumerate(R.HEADS)]
    if stats is not None:
        stats.update(st)
    return torch.cat(cols, 1)


def loss_and_grads(params, x, edge_index, edge_weight, mask_t, inst_t, edge_t, heads, nc, rates=(0.0, 0.0, 0.0), seed=0, batch=False,
                   weights=(1.0, 1.0, 1.0), dtype=torch.float64, momentum=BR.MOMENTUM, want_grads=True, masks=None):
    """Returns (losses float [4], {name: gradient} for the 32 trainable parameters, flip margin over the nine taps, batch_stats
    [4, 2, C] or None, {name: updated running statistic} or None) -- the last two under batch statistics only."""
    n = x.shape[0]
    src, dst, w = RO.with_self_loops(n, edge_index, edge_weight)
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    names = trainable_names()
    for k in names:
        P[k].requires_grad_(want_grads)
    taps, st = [], {}
    logits = forward(P, torch.tensor(x, dtype=dtype), torch.tensor(src), torch.tensor(dst), torch.tensor(w, dtype=dtype), heads, rates, seed,
                     batch, taps, momentum, st, masks)
    ls = losses(logits, torch.tensor(mask_t, dtype=torch.int64), torch.tensor(inst_t, dtype=torch.int64), torch.tensor(edge_t, dtype=dtype),
                weights, nc)
    grads = {}
    if want_grads:
        gs = torch.autograd.grad(ls[0], [P[k] for k in names], allow_unused=True)
        grads = {k: (np.zeros(P[k].shape) if g is None else g.double().numpy()) for k, g in zip(names, gs)}
    bs, running = BR.stats_arrays(st) if batch else (None, None)
    return [float(v.detach()) for v in ls], grads, BR.margin_of(taps), bs, running
