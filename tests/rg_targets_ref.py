"""include/camo_rg_targets.h restated in numpy, int64 throughout: the checker of ``camo_rg_node_targets``.

PARITY UNPINNED (the reference's CODDataset cannot be read here): the header is the definition, this file says the same thing a
second time with ``np.add.at`` and plain comparisons, and the kernels are held to it for exact equality.
"""
import numpy as np


def positive(gt):
    """A ground-truth byte is positive above 127; a bool mask is its own answer."""
    gt = np.asarray(gt)
    return gt.astype(bool) if gt.dtype == np.bool_ else gt.astype(np.int64) > 127


def mask_boundary(gt_mask):
    """[N, H, W] bool: positive pixels with at least one 4-neighbour inside the image that is not positive."""
    p = positive(gt_mask)
    out = np.zeros_like(p)
    out[:, 1:, :] |= p[:, 1:, :] & ~p[:, :-1, :]
    out[:, :-1, :] |= p[:, :-1, :] & ~p[:, 1:, :]
    out[:, :, 1:] |= p[:, :, 1:] & ~p[:, :, :-1]
    out[:, :, :-1] |= p[:, :, :-1] & ~p[:, :, 1:]
    return out


def pixel_nodes(segments, region_map, node_off, n_nodes):
    """[N, H, W] int64: the node of every pixel, -1 where the pixel takes no part."""
    seg, rmap, off = np.asarray(segments, np.int64), np.asarray(region_map, np.int64), np.asarray(node_off, np.int64)
    N, lb = rmap.shape
    ok = (seg >= 0) & (seg < lb)
    r = np.take_along_axis(rmap.reshape(N, 1, lb), np.where(ok, seg, 0).reshape(N, 1, -1), 2).reshape(seg.shape)
    v = off[:N].reshape(N, 1, 1) + r
    ok &= (r >= 0) & (v >= 0) & (v < n_nodes)
    return np.where(ok, v, -1)


def node_counts(segments, region_map, node_off, gt_mask, gt_instance=None, gt_edge=None, n_nodes=None):
    """counts int64 [n_nodes, 4] = pixels, mask-positive, instance-positive, edge pixels of every node."""
    n_nodes = int(np.asarray(node_off)[-1]) if n_nodes is None else int(n_nodes)
    v = pixel_nodes(segments, region_map, node_off, n_nodes)
    m = positive(gt_mask)
    inst = m if gt_instance is None else positive(gt_instance)
    edge = mask_boundary(gt_mask) if gt_edge is None else positive(gt_edge)
    counts = np.zeros((n_nodes, 4), np.int64)
    take = v >= 0
    for q, what in enumerate((np.ones_like(m), m, inst, edge)):
        np.add.at(counts[:, q], v[take], what[take].astype(np.int64))
    return counts


def vote(pos, pix, band):
    pos, pix = np.asarray(pos, np.int64), np.asarray(pix, np.int64)
    t = np.full(pix.shape, -1, np.int64)
    t[1000 * pos <= (500 - band) * pix] = 0
    t[1000 * pos > (500 + band) * pix] = 1
    t[pix == 0] = -1
    return t


def targets_from_counts(counts, band_permille=0, edge_min_pixels=1):
    """(mask_t int32 [n], inst_t int32 [n], edge_t float32 [n]) from counts [n, 4]."""
    c = np.asarray(counts, np.int64)
    pix = c[:, 0]
    edge = np.where(pix == 0, -1.0, (c[:, 3] >= edge_min_pixels).astype(np.float64)).astype(np.float32)
    return vote(c[:, 1], pix, band_permille).astype(np.int32), vote(c[:, 2], pix, band_permille).astype(np.int32), edge


def node_targets(segments, region_map, node_off, gt_mask, gt_instance=None, gt_edge=None, band_permille=0, edge_min_pixels=1, n_nodes=None):
    """(mask_t, inst_t, edge_t, counts int32 [n_nodes, 4]): the four outputs of camo_rg_node_targets."""
    counts = node_counts(segments, region_map, node_off, gt_mask, gt_instance, gt_edge, n_nodes)
    return targets_from_counts(counts, band_permille, edge_min_pixels) + (counts.astype(np.int32),)


def compact_region_map(segments, label_bound):
    """What camo_rg_region_graph_batch gives for labels in range: per image, the labels that occur ranked in increasing order, -1
    for the others; and node_off [N + 1]."""
    seg = np.asarray(segments)
    N = seg.shape[0]
    rmap = np.full((N, label_bound), -1, np.int32)
    off = np.zeros(N + 1, np.int32)
    for i in range(N):
        labs = np.unique(seg[i][(seg[i] >= 0) & (seg[i] < label_bound)])
        rmap[i, labs] = np.arange(labs.size, dtype=np.int32)
        off[i + 1] = off[i] + labs.size
    return rmap, off
