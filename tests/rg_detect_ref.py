"""numpy restatement of include/camo_rg_detect.h -- TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED (the reference tree, torch_geometric,
scikit-image and an RG checkpoint are absent): the header's text is the definition, this file says it again in float64 on the
fp32 inputs, and tests/test_rg_detect.py holds the HIP kernels to it."""
import numpy as np

HEADS = ("fc_mask", "fc_instance", "fc_edge")
FIX = 2.0 ** 32


def head_specs(hidden=128, num_classes=2):
    """(name, shape) of the twelve head parameters in state_dict order = the header's CAMO_RGD_* order."""
    out = []
    for h in HEADS:
        c = 1 if h == "fc_edge" else num_classes
        out += [(f"{h}_1.weight", (hidden // 2, hidden)), (f"{h}_1.bias", (hidden // 2,)), (f"{h}_2.weight", (c, hidden // 2)), (f"{h}_2.bias", (c,))]
    return out


def make_head_params(seed=0, hidden=128, num_classes=2):
    """Weights N(0, 1) / sqrt(fan_in), biases 0.05 N(0, 1): the style of the GNN checker's make_params."""
    rs = np.random.RandomState(seed)
    p = {}
    for name, shape in head_specs(hidden, num_classes):
        if name.endswith("bias"):
            p[name] = (0.05 * rs.standard_normal(shape)).astype(np.float32)
        else:
            p[name] = (rs.standard_normal(shape) / np.sqrt(shape[-1])).astype(np.float32)
    return p


def heads(p, emb):
    """logits [n, 2 c + 1] in float64: mask | instance | edge."""
    e = np.asarray(emb, np.float64)
    cols = []
    for h in HEADS:
        z = np.maximum(e @ p[f"{h}_1.weight"].astype(np.float64).T + p[f"{h}_1.bias"].astype(np.float64), 0.0)
        cols.append(z @ p[f"{h}_2.weight"].astype(np.float64).T + p[f"{h}_2.bias"].astype(np.float64))
    return np.concatenate(cols, axis=1)


def probabilities(logits, num_classes):
    """[n, 3] in float64: softmax(l_mask)[1], softmax(l_instance)[1], sigmoid(l_edge)."""
    l = np.asarray(logits, np.float64)
    out = np.empty((l.shape[0], 3))
    for h in range(2):
        lh = l[:, h * num_classes:(h + 1) * num_classes]
        ex = np.exp(lh - lh.max(axis=1, keepdims=True))
        out[:, h] = ex[:, 1] / ex.sum(axis=1)
    out[:, 2] = 1.0 / (1.0 + np.exp(-l[:, 2 * num_classes]))
    return out


def region_map_of(segments, label_bound):
    """(region_map int32 [N, label_bound], node_off int32 [N + 1]) of label maps [N, H, W]: the labels present in [0, label_bound), in
    increasing order, get 0, 1, ...; the others -1 (what the batched graph construction returns)."""
    N = segments.shape[0]
    rmap = np.full((N, label_bound), -1, np.int32)
    off = [0]
    for i in range(N):
        present = np.unique(segments[i])
        present = present[(present >= 0) & (present < label_bound)]
        rmap[i, present] = np.arange(len(present), dtype=np.int32)
        off.append(off[-1] + len(present))
    return rmap, np.asarray(off, np.int32)


def paint(values, segments, region_map, node_off, fill=0.0):
    """maps [N, C, H, W] float32: a pure gather, so the bits of `values` (or of float32(fill))."""
    values = np.asarray(values, np.float32)
    N, H, W = segments.shape
    L = region_map.shape[1]
    out = np.full((N, values.shape[1], H, W), np.float32(fill), np.float32)
    for i in range(N):
        s = segments[i]
        ok = (s >= 0) & (s < L)
        r = np.where(ok, region_map[i][np.clip(s, 0, L - 1)], -1)
        row = int(node_off[i]) + r.astype(np.int64)
        ok = (r >= 0) & (row < values.shape[0])
        out[i][:, ok] = values[row[ok]].T
    return out


def counts(pred, gt, threshold=0.5):
    """int64 [N, 5] = TP, FP, FN, TN, A of pred float32 [N, H, W] against gt uint8 [N, H, W]; A = sum rint(|pred - g| 2^32) with the
    difference in float64 (exact for fp32 inputs in [0, 1]; rint and llrint both round half to even)."""
    pred = np.asarray(pred, np.float32)
    N = pred.shape[0]
    out = np.zeros((N, 5), np.int64)
    for i in range(N):
        pp = pred[i] > np.float32(threshold)
        gp = np.asarray(gt[i]) > 127
        a = np.rint(np.abs(pred[i].astype(np.float64) - gp.astype(np.float64)) * FIX).astype(np.int64)
        out[i] = [(pp & gp).sum(), (pp & ~gp).sum(), (~pp & gp).sum(), (~pp & ~gp).sum(), a.sum()]
    return out


def ratios(row, H, W):
    """The header's conventions, float64."""
    tp, fp, fn, tn, a = (int(v) for v in row)
    p = tp / (tp + fp) if tp + fp else 0.0
    r = tp / (tp + fn) if tp + fn else 0.0
    return {"iou": tp / (tp + fp + fn) if tp + fp + fn else 1.0, "dice": 2 * tp / (2 * tp + fp + fn) if tp + fp + fn else 1.0,
            "precision": p, "recall": r, "f1": 2 * p * r / (p + r) if p + r else 0.0, "accuracy": (tp + tn) / (H * W),
            "mae": a / FIX / (H * W)}
