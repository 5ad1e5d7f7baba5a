"""include/camo_rg_pixel_loss.h restated -- TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED (the reference's trainer cannot be read here):
the header is the definition.  This file says it again three times:

  * the node weights in numpy, int64 throughout (``pixel_q``, ``node_weights``): the checker of ``camo_rg_pixel_weights``, exact;
  * the loss in its PIXEL form (``pixel_form``): F3Net's structure loss written as its authors wrote it -- avg_pool2d, a weighted
    binary_cross_entropy_with_logits, a weighted soft IoU -- on the map painted from the node logits, over the pixels that take part;
  * the loss in its NODE form (``node_form``): the header's sums over (A_v, B_v), in any dtype.

``loss_and_grads`` puts either form behind the forward of tests/rg_train_drop_ref.py (rg_train_ref's, or with batch statistics and
dropout) and takes the gradients of the 32 parameters from autograd."""
import numpy as np
import torch

from oracle import rg_gnn_oracle as RO

import rg_targets_ref as TG
import rg_train_bn_ref as BR
import rg_train_drop_ref as DR
import rg_train_ref as TR

RADIUS, GAIN = 15, 5          # the defaults (F3Net: a 31 x 31 window and a gain of 5)


def box_sum(g, radius):
    """S int64 [N, H, W]: the sum of g over the (2 r + 1)^2 window clipped to the image, by a summed-area table."""
    g = np.asarray(g, np.int64)
    N, H, W = g.shape
    r = int(radius)
    sat = np.zeros((N, H + 1, W + 1), np.int64)
    sat[:, 1:, 1:] = g.cumsum(1).cumsum(2)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return sat[:, y1][:, :, x1] - sat[:, y0][:, :, x1] - sat[:, y1][:, :, x0] + sat[:, y0][:, :, x0]


def pixel_q(gt_mask, radius=RADIUS, gain=GAIN):
    """(q int64 [N, H, W], g int64 [N, H, W], K): q = K + gain |S - K g|."""
    g = TG.positive(gt_mask).astype(np.int64)
    K = (2 * int(radius) + 1) ** 2
    return K + int(gain) * np.abs(box_sum(g, radius) - K * g), g, K


def node_weights(segments, region_map, node_off, gt_mask, radius=RADIUS, gain=GAIN, n_nodes=None):
    """node_w int64 [n_nodes, 2] = (A_v, B_v) = (sum q, sum q g) over the pixels of every node that take part."""
    n_nodes = int(np.asarray(node_off)[-1]) if n_nodes is None else int(n_nodes)
    v = TG.pixel_nodes(segments, region_map, node_off, n_nodes)
    q, g, _ = pixel_q(gt_mask, radius, gain)
    out = np.zeros((n_nodes, 2), np.int64)
    take = v >= 0
    np.add.at(out[:, 0], v[take], q[take])
    np.add.at(out[:, 1], v[take], (q * g)[take])
    return out


def pixel_form(z, segments, region_map, node_off, gt_mask, radius=RADIUS, gain=GAIN):
    """(P, mean wbce, mean wiou) of node logit differences z [n] (a torch tensor; the result is in its dtype and differentiable):
    F3Net's structure_loss, image by image, on pred = z painted through the label map, over the pixels that take part.  An image
    without such a pixel is left out; no image left: zeros."""
    F = torch.nn.functional
    v = TG.pixel_nodes(segments, region_map, node_off, z.shape[0])
    g = torch.from_numpy(TG.positive(gt_mask).astype(np.float64)).to(z.dtype)
    win = 2 * int(radius) + 1
    weit = 1 + gain * torch.abs(F.avg_pool2d(g[:, None], kernel_size=win, stride=1, padding=int(radius))[:, 0] - g)
    bces, ious = [], []
    for i in range(v.shape[0]):
        take = torch.from_numpy(v[i] >= 0)
        if not bool(take.any()):
            continue
        pred = z[torch.from_numpy(np.where(v[i] >= 0, v[i], 0))][take]
        mask, w = g[i][take], weit[i][take]
        wbce = (w * F.binary_cross_entropy_with_logits(pred, mask, reduction="none")).sum() / w.sum()
        p = torch.sigmoid(pred)
        inter, union = (p * mask * w).sum(), ((p + mask) * w).sum()
        bces.append(wbce)
        ious.append(1 - (inter + 1) / (union - inter + 1))
    if not bces:
        return z.sum() * 0, z.sum() * 0, z.sum() * 0
    b, u = torch.stack(bces).mean(), torch.stack(ious).mean()
    return b + u, b, u


def node_form(z, node_w, node_off, radius=RADIUS):
    """The same three figures from node_w [n, 2] (A, B) and node_off, as the header writes them, in z's dtype.  node_off is clamped
    to [0, n] and a decreasing pair is an empty image, as on the device."""
    n = z.shape[0]
    A = torch.from_numpy(np.asarray(node_w, np.int64)[:, 0].astype(np.float64)).to(z.dtype)
    B = torch.from_numpy(np.asarray(node_w, np.int64)[:, 1].astype(np.float64)).to(z.dtype)
    K = float((2 * int(radius) + 1) ** 2)
    off = np.clip(np.asarray(node_off, np.int64), 0, n)
    p = torch.sigmoid(z)
    sp_pos, sp_neg = torch.nn.functional.softplus(z), torch.nn.functional.softplus(-z)
    bces, ious = [], []
    for i in range(len(off) - 1):
        sl = slice(int(off[i]), int(max(off[i + 1], off[i])))
        SA = A[sl].sum()
        if not float(SA) > 0:
            continue
        I = (p[sl] * B[sl]).sum()
        D = (p[sl] * A[sl]).sum() + B[sl].sum() - I + K
        bces.append((B[sl] * sp_neg[sl] + (A[sl] - B[sl]) * sp_pos[sl]).sum() / SA)
        ious.append(1 - (I + K) / D)
    if not bces:
        return z.sum() * 0, z.sum() * 0, z.sum() * 0
    b, u = torch.stack(bces).mean(), torch.stack(ious).mean()
    return b + u, b, u


def node_gradient(z, node_w, node_off, radius=RADIUS):
    """dP/dz [n] in float64 by the header's closed form (not autograd)."""
    z = np.asarray(z, np.float64)
    n = z.shape[0]
    A, B = (np.asarray(node_w, np.int64)[:, k].astype(np.float64) for k in (0, 1))
    K = float((2 * int(radius) + 1) ** 2)
    off = np.clip(np.asarray(node_off, np.int64), 0, n)
    p = 1.0 / (1.0 + np.exp(-z))
    out = np.zeros(n)
    left = [i for i in range(len(off) - 1) if A[off[i]:max(off[i + 1], off[i])].sum() > 0]
    for i in left:
        sl = slice(int(off[i]), int(max(off[i + 1], off[i])))
        SA, I = A[sl].sum(), (p[sl] * B[sl]).sum()
        D = (p[sl] * A[sl]).sum() + B[sl].sum() - I + K
        out[sl] += ((A[sl] * p[sl] - B[sl]) / SA - p[sl] * (1 - p[sl]) * (B[sl] * D - (I + K) * (A[sl] - B[sl])) / D ** 2) / len(left)
    return out


def loss_and_grads(params, x, edge_index, edge_weight, mask_t, inst_t, edge_t, heads, nc, pixel, w_pixel, weights=(1.0, 1.0, 1.0),
                   dtype=torch.float64, rates=(0.0, 0.0, 0.0), seed=0, batch=False):
    """(losses float [6] = total, mask, instance, edge, mean wbce, mean wiou; {name: gradient} of the 32 trainable parameters; flip
    margin).  `pixel`: a function z -> (P, wbce, wiou), one of the two forms above with its arrays bound.  The forward is
    rg_train_drop_ref's: rg_train_ref's at rates 0 and batch False."""
    assert nc == 2
    n = x.shape[0]
    src, dst, w = RO.with_self_loops(n, edge_index, edge_weight)
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    names = TR.trainable_names()
    for k in names:
        P[k].requires_grad_(True)
    taps = []
    logits = DR.forward(P, torch.tensor(x, dtype=dtype), torch.tensor(src), torch.tensor(dst), torch.tensor(w, dtype=dtype), heads, rates, seed,
                        batch, taps)
    ls = TR.losses(logits, torch.tensor(mask_t, dtype=torch.int64), torch.tensor(inst_t, dtype=torch.int64), torch.tensor(edge_t, dtype=dtype),
                   weights, nc)
    pt, wbce, wiou = pixel(logits[:, 1] - logits[:, 0])
    total = ls[0] + w_pixel * pt
    grads = torch.autograd.grad(total, [P[k] for k in names], allow_unused=True)
    grads = {k: (np.zeros(P[k].shape) if g is None else g.double().numpy()) for k, g in zip(names, grads)}
    return [float(v.detach()) for v in [total] + ls[1:] + [wbce, wiou]], grads, BR.margin_of(taps)
