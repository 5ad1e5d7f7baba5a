"""torch restatement of include/camo_rg_train.h -- TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED (the reference tree, torch_geometric and
an RG checkpoint are absent): the header's text is the definition; this file says the forward and the loss again in torch, in float64
on the fp32 inputs (or in float32, to measure what fp32 arithmetic alone costs), and takes the gradients from autograd.
tests/test_rg_train.py ties its logits to oracle/rg_gnn_oracle.py + tests/rg_detect_ref.py and holds the HIP kernels to its gradients."""
import numpy as np
import torch

from oracle import rg_gnn_oracle as RO

import rg_detect_ref as R

EPS = float(np.float32(1e-5))
FLIP_MARGIN = 1e-4          # 5 x the 2e-5 the forward is held to


def trainable_names():
    """The 32 trainable parameters in the order of the gradient table (include/camo_rg_train.h)."""
    names = ["conv1.att_src", "conv1.att_dst", "conv1.bias", "conv1.lin.weight", "bn1.weight", "bn1.bias"]
    for k in (2, 3, 4):
        names += [f"conv{k}.bias", f"conv{k}.lin.weight", f"bn{k}.weight", f"bn{k}.bias"]
    names += ["fc_shared.weight", "fc_shared.bias"]
    return names + [n for n, _ in R.head_specs()]


def forward(P, x, src, dst, w, heads, taps=None):
    """logits [n, 2 c + 1] = mask | instance | edge from the parameter dict P (torch tensors of one dtype), the features x and the
    edge list WITH its self-loops (RO.with_self_loops).  `taps`: a list that receives every pre-activation whose sign the gradient
    depends on (the attention scores per edge, the four batch-norm outputs, the fc_shared output, the heads' hidden layers)."""
    n, hidden = x.shape[0], P["conv1.bias"].shape[0]
    tap = (lambda t: taps.append(t.detach())) if taps is not None else (lambda t: None)

    def bn(v, k):
        return (v - P[f"bn{k}.running_mean"]) / torch.sqrt(P[f"bn{k}.running_var"] + EPS) * P[f"bn{k}.weight"] + P[f"bn{k}.bias"]

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
    return torch.cat(cols, 1)


def cross_entropy(l, t):
    """Mean over the nodes with t in [0, classes) of logsumexp(l) - l[t] (the header: any other target is ignored); 0 (with zero
    gradient) when there is none."""
    keep = (t >= 0) & (t < l.shape[1])
    if int(keep.sum()) == 0:
        return l.sum() * 0
    lk = l[keep]
    mx = lk.max(1, keepdim=True).values.detach()
    return (mx[:, 0] + torch.log(torch.exp(lk - mx).sum(1)) - lk.gather(1, t[keep, None])[:, 0]).mean()


def bce_with_logits(z, t):
    """Mean over the nodes with t >= 0 of max(z, 0) - z t + log(1 + exp(-|z|)); 0 when there is none."""
    keep = t >= 0
    if int(keep.sum()) == 0:
        return z.sum() * 0
    zk, tk = z[keep], t[keep].to(z.dtype)
    return (zk.clamp_min(0) - zk * tk + torch.log(1 + torch.exp(-zk.abs()))).mean()


def losses(logits, mask_t, inst_t, edge_t, weights, nc):
    """[total, mask, instance, edge]"""
    lm = cross_entropy(logits[:, :nc], mask_t)
    li = cross_entropy(logits[:, nc:2 * nc], inst_t)
    le = bce_with_logits(logits[:, 2 * nc], edge_t)
    return [weights[0] * lm + weights[1] * li + weights[2] * le, lm, li, le]


def loss_and_grads(params, x, edge_index, edge_weight, mask_t, inst_t, edge_t, heads, nc, weights=(1.0, 1.0, 1.0), dtype=torch.float64,
                   probe=None):
    """params: dict name -> fp32 numpy array (embedding path + heads, running statistics included).  Returns
    (losses float [4], {name: gradient numpy array} for the 32 trainable parameters, min over the taps of min|t| / max|t|).
    `probe`: a dict that receives "max_score" = max|s| and "top_score" = max s over the attention scores, and "max_logit" = max|logit|."""
    n = x.shape[0]
    src, dst, w = RO.with_self_loops(n, edge_index, edge_weight)
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    names = trainable_names()
    for k in names:
        P[k].requires_grad_(True)
    taps = []
    logits = forward(P, torch.tensor(x, dtype=dtype), torch.tensor(src), torch.tensor(dst), torch.tensor(w, dtype=dtype), heads, taps)
    ls = losses(logits, torch.tensor(mask_t, dtype=torch.int64), torch.tensor(inst_t, dtype=torch.int64), torch.tensor(edge_t, dtype=dtype),
                weights, nc)
    grads = torch.autograd.grad(ls[0], [P[k] for k in names], allow_unused=True)
    grads = {k: (np.zeros(P[k].shape) if g is None else g.numpy()) for k, g in zip(names, grads)}
    margin = min(float(t.abs().min() / t.abs().max()) for t in taps if t.numel())
    if probe is not None:
        probe["max_score"], probe["top_score"] = float(taps[0].abs().max()), float(taps[0].max())
        probe["max_logit"] = float(logits.detach().abs().max())
    return [float(v.detach()) for v in ls], grads, margin
