"""torch restatement of include/camo_rg_train_bn.h -- TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED (the reference tree, torch_geometric
and an RG checkpoint are absent): the header's text is the definition.  This file says tests/rg_train_ref.py's forward again with every
BatchNorm1d on the statistics of the call's own nodes (biased variance, eps 1e-5) and the running statistics updated with the unbiased
one; the loss is rg_train_ref's, the gradients are autograd's.  tests/test_rg_train_bn.py ties the batch-norm step to
torch.nn.functional.batch_norm(training=True) and the rest to rg_train_ref.forward, and holds the HIP kernels to these gradients."""
import numpy as np
import torch

from oracle import rg_gnn_oracle as RO

import rg_detect_ref as R
import rg_train_ref as TR
from rg_train_ref import EPS, FLIP_MARGIN, losses, trainable_names  # noqa: F401  (the loss and the gradient table are unchanged)

MOMENTUM = 0.1              # BatchNorm1d's default


def bn_step(z, weight, bias, running_mean, running_var, momentum, one_pass=False):
    """z [N, C] -> (weight * xhat + bias, mu, biased var, new running_mean, new running_var).  `one_pass`: the variance as
    E[z^2] - mu^2 -- what the kernels must NOT do; only the "offset" case's demonstration uses it."""
    n = z.shape[0]
    mu = z.mean(0)
    var = ((z * z).mean(0) - mu * mu) if one_pass else ((z - mu) ** 2).mean(0)
    xhat = (z - mu) / torch.sqrt(var + EPS)
    new_mean = (1 - momentum) * running_mean + momentum * mu.detach()
    new_var = (1 - momentum) * running_var + momentum * var.detach() * (n / (n - 1))
    return xhat * weight + bias, mu.detach(), var.detach(), new_mean, new_var


def forward(P, x, src, dst, w, heads, taps=None, momentum=MOMENTUM, stats=None, one_pass=False):
    """rg_train_ref.forward with batch statistics.  `stats`: a dict that receives "mu" and "var" (lists of four [C] tensors) and
    "running" (name -> updated tensor, the eight running statistics)."""
    n, hidden = x.shape[0], P["conv1.bias"].shape[0]
    tap = (lambda t: taps.append(t.detach())) if taps is not None else (lambda t: None)
    st = {"mu": [], "var": [], "running": {}}

    def bn(v, k):
        y, mu, var, rm, rv = bn_step(v, P[f"bn{k}.weight"], P[f"bn{k}.bias"], P[f"bn{k}.running_mean"], P[f"bn{k}.running_var"], momentum,
                                     one_pass)
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
    h = torch.relu(y)
    deg = torch.zeros(n, dtype=x.dtype).index_add(0, dst, w)
    dinv = torch.where(deg > 0, deg.clamp_min(1e-30).rsqrt(), torch.zeros_like(deg))
    norm = dinv[src] * w * dinv[dst]
    for k in (2, 3, 4):
        xw = h @ P[f"conv{k}.lin.weight"].T
        y = bn(torch.zeros_like(xw).index_add(0, dst, norm[:, None] * xw[src]) + P[f"conv{k}.bias"], k)
        tap(y)
        h = torch.relu(y)
    y = h @ P["fc_shared.weight"].T + P["fc_shared.bias"]
    tap(y)
    emb = torch.relu(y)
    cols = []
    for name in R.HEADS:
        y = emb @ P[f"{name}_1.weight"].T + P[f"{name}_1.bias"]
        tap(y)
        cols.append(torch.relu(y) @ P[f"{name}_2.weight"].T + P[f"{name}_2.bias"])
    if stats is not None:
        stats.update(st)
    return torch.cat(cols, 1)


def margin_of(taps):
    return min(float(t.abs().min() / t.abs().max()) for t in taps if t.numel())


def stats_arrays(st):
    """(batch_stats float64 [4, 2, C] = mu, biased var per layer; {name: updated running statistic})"""
    bs = np.stack([np.stack([mu.double().numpy(), var.double().numpy()]) for mu, var in zip(st["mu"], st["var"])])
    return bs, {k: v.detach().double().numpy() for k, v in st["running"].items()}


def loss_and_grads(params, x, edge_index, edge_weight, mask_t, inst_t, edge_t, heads, nc, weights=(1.0, 1.0, 1.0), dtype=torch.float64,
                   momentum=MOMENTUM, one_pass=False, want_grads=True):
    """rg_train_ref.loss_and_grads under batch statistics.  Returns (losses float [4], {name: gradient} for the 32 trainable
    parameters, flip margin over the nine taps, batch_stats [4, 2, C], {name: updated running statistic})."""
    n = x.shape[0]
    src, dst, w = RO.with_self_loops(n, edge_index, edge_weight)
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    names = trainable_names()
    for k in names:
        P[k].requires_grad_(want_grads)
    taps, st = [], {}
    logits = forward(P, torch.tensor(x, dtype=dtype), torch.tensor(src), torch.tensor(dst), torch.tensor(w, dtype=dtype), heads, taps,
                     momentum, st, one_pass)
    ls = losses(logits, torch.tensor(mask_t, dtype=torch.int64), torch.tensor(inst_t, dtype=torch.int64), torch.tensor(edge_t, dtype=dtype),
                weights, nc)
    grads = {}
    if want_grads:
        gs = torch.autograd.grad(ls[0], [P[k] for k in names], allow_unused=True)
        grads = {k: (np.zeros(P[k].shape) if g is None else g.double().numpy()) for k, g in zip(names, gs)}
    bs, running = stats_arrays(st)
    return [float(v.detach()) for v in ls], grads, margin_of(taps), bs, running
