"""Region-Graph construction and GNN embedding path on MI355X.

``RegionGraphGNN`` keeps the reference module's name, constructor and ``state_dict`` keys
(models/region_graph/extract_rg_embeddings.py:27-52), so ``best_model.pth`` loads with ``strict=True``
(test_multimodal.py:420-423); ``extract_node_embeddings(data)`` (:94-122) -- the call that feeds the fusion model at
inference -- runs as HIP kernels behind ``camo_rg_node_embeddings`` (include/camo_rg_gnn.h).  The graph layers are
torch_geometric's in the reference; the published algorithms they are restated from and the CPU checker the kernels are
tested against are named in include/camo_rg_gnn.h (PARITY UNPINNED: no PyG here, no RG weights or fixtures shipped).  The node-classification ``forward``
runs in eval mode (``camo_rg_node_heads``, include/camo_rg_detect.h; the detector built on it is rg_detect.py and pipeline.py).  ``loss_and_gradients``
gives the loss on the heads and every parameter's gradient with the batch-norm statistics frozen (``camo_rg_loss_backward``,
include/camo_rg_train.h) or, with ``batch_stats=True``, on the statistics of the call's own nodes, the running statistics updated
(``camo_rg_loss_backward_bn``, include/camo_rg_train_bn.h), and with ``dropout=`` under inverted dropout at the model's eight sites
(``camo_rg_loss_backward_drop``, include/camo_rg_train_drop.h), and with ``pixel=`` plus the structure loss on the painted mask
(``camo_rg_loss_backward_pixel``, include/camo_rg_pixel_loss.h).  A training-mode logits entry is not built: ``forward`` in training
mode raises.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import _ptr, _stream_ptr, call, workspace


def _as_tensor(value, device):
    """A tensor is used where it is; anything else is placed on ``device``."""
    return value if isinstance(value, torch.Tensor) else torch.as_tensor(value).to(torch.device(device))


def _image_batch(img, single_ok=False):
    """A tensor of images as (contiguous fp32 [N, H, W, 3], whether it came as one [H, W, 3] image, which only ``single_ok``
    allows); any other shape raises.  Where the tensor lives is the caller's check, before or after this one."""
    single = single_ok and img.dim() == 3
    if single:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[3] != 3 or img.numel() == 0:
        raise ValueError(f"need images {'[H, W, 3] or ' if single_ok else ''}[N, H, W, 3], got {tuple(img.shape)}")
    return img.to(torch.float32).contiguous(), single


def build_target_csr_device(num_nodes, edge_index, edge_weight=None):
    """The same CSR as ``build_target_csr`` built by the library (``camo_rg_build_csr``: counting sort by target, four
    small launches instead of a chain of torch index kernels); a row's edges after its leading self-loop come in no
    particular order.  Returns (rowptr int32 [N+1], col int32 [E+N], w fp32 [E+N])."""
    _lib.require_device(edge_index, "edge_index")
    dev = edge_index.device
    ei = edge_index.to(torch.int64).contiguous()
    E = ei.shape[1]
    ew = None if edge_weight is None else edge_weight.reshape(-1).to(torch.float32).contiguous()
    scratch = torch.empty(3 * num_nodes, dtype=torch.int32, device=dev)
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E + num_nodes, dtype=torch.int32, device=dev)
    w = torch.empty(E + num_nodes, dtype=torch.float32, device=dev)
    rc = _lib.lib().camo_rg_build_csr(_ptr(ei), _ptr(ew), num_nodes, E, _ptr(scratch), _ptr(rowptr), _ptr(col), _ptr(w), _stream_ptr())
    _lib.check(rc, "camo_rg_build_csr")
    return rowptr, col, w


def build_target_csr(num_nodes, edge_index, edge_weight=None):
    """edge_index [2, E] (row 0 = source j, row 1 = target i, PyG convention), edge_weight [E] or None ->
    (rowptr int32 [N+1], col int32 [E'], w fp32 [E']) sorted by target with exactly one self-loop per node: existing
    self-loops keep their weight, missing ones get weight 1 (PyG ``add_remaining_self_loops``; GATConv's
    remove-then-add gives the same structure and ignores weights).  Index plumbing on the tensors' device."""
    dev = edge_index.device
    src, dst = edge_index[0].long(), edge_index[1].long()
    w = torch.ones(src.shape[0], dtype=torch.float32, device=dev) if edge_weight is None else edge_weight.reshape(-1).to(torch.float32)
    loop = src == dst
    lw = torch.ones(num_nodes, dtype=torch.float32, device=dev)
    lw[src[loop]] = w[loop]
    ar = torch.arange(num_nodes, device=dev)
    src = torch.cat([src[~loop], ar]); dst = torch.cat([dst[~loop], ar]); w = torch.cat([w[~loop], lw])
    order = torch.argsort(dst * num_nodes + src, stable=True)
    rowptr = torch.zeros(num_nodes + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=num_nodes), 0)
    return rowptr.to(torch.int32), src[order].to(torch.int32).contiguous(), w[order].contiguous()


class RegionGraphData:
    """What the reference's ``create_region_graph`` returns as a torch_geometric ``Data`` (extract_rg_embeddings.py:239-243):
    ``x`` [n, 15], ``edge_index`` [2, E] int64, ``edge_attr`` [E, 1]; duck-typed for ``extract_node_embeddings``."""

    def __init__(self, x, edge_index, edge_attr):
        self.x, self.edge_index, self.edge_attr = x, edge_index, edge_attr

    def to(self, device):
        return RegionGraphData(self.x.to(device), self.edge_index.to(device), self.edge_attr.to(device))

    cpu = lambda self: self.to("cpu")  # noqa: E731


class RegionGraphBatch:
    """The region graphs of N images as ONE block-diagonal graph (torch_geometric's ``Batch``): ``x`` [n, 15] with the regions of
    image k in rows ``node_offsets[k] : node_offsets[k + 1]``, ``edge_index`` [2, E] int64 with global node indices (image k's edges
    in columns ``edge_offsets[k] : edge_offsets[k + 1]``), ``edge_attr`` [E, 1], ``batch`` [n] int32 image index of every node,
    ``num_graphs``.  The offsets are host lists of N + 1 integers.  Duck-typed for ``extract_node_embeddings`` /
    ``extract_graph_embedding``."""

    def __init__(self, x, edge_index, edge_attr, batch, node_offsets, edge_offsets):
        self.x, self.edge_index, self.edge_attr, self.batch = x, edge_index, edge_attr, batch
        self.node_offsets, self.edge_offsets = list(node_offsets), list(edge_offsets)
        self.num_graphs = len(self.node_offsets) - 1

    def to(self, device):
        return RegionGraphBatch(self.x.to(device), self.edge_index.to(device), self.edge_attr.to(device), self.batch.to(device),
                                self.node_offsets, self.edge_offsets)

    cpu = lambda self: self.to("cpu")  # noqa: E731

    def graphs(self):
        """Per-image ``RegionGraphData`` (rows of ``x`` and ``edge_attr`` are views; edge indices are local to the image)."""
        no, eo = self.node_offsets, self.edge_offsets
        return [RegionGraphData(self.x[no[k]:no[k + 1]], self.edge_index[:, eo[k]:eo[k + 1]] - no[k], self.edge_attr[eo[k]:eo[k + 1]])
                for k in range(self.num_graphs)]


def canny_edges(images, sigma=2.0, low_threshold=0.1, high_threshold=0.2, device="cuda", return_gradients=False):
    """``skimage.feature.canny(gray, sigma=2)`` of the reference (extract_rg_embeddings.py:151-152, luma :151 included) on the
    device (``camo_canny``, include/camo_canny.h): ``images`` [H, W, 3] or [N, H, W, 3] float in [0, 1] -> bool tensor [H, W]
    or [N, H, W] on the device; with ``return_gradients`` also the fp32 gradients [N, 3, H, W] = gi, gj, magnitude ([3, H, W]
    for one image).  A tensor is used where it is (``device`` places other inputs) and must be on a HIP device.  PARITY UNPINNED,
    see the header."""
    img = _as_tensor(images, device)
    _lib.require_device(img, "images")
    img, single = _image_batch(img, single_ok=True)
    dev = img.device
    N, H, W = img.shape[:3]
    ws, nbytes = workspace("camo_canny_workspace_bytes", N, H, W, device=dev)
    edges = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    grad = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev) if return_gradients else None
    call("camo_canny", dev, _ptr(img), N, H, W, float(sigma), float(low_threshold), float(high_threshold), _ptr(ws), nbytes, _ptr(edges),
         _ptr(grad), _stream_ptr(dev))
    edges = edges.to(torch.bool)
    if single:
        edges, grad = edges[0], (None if grad is None else grad[0])
    return (edges, grad) if return_gradients else edges


def create_region_graph_from_segments(image, segments, edges_canny=None, device="cuda", edge_capacity=None):
    """The body of ``create_region_graph`` (extract_rg_embeddings.py:146-246) between its skimage calls, on the device
    (``camo_rg_region_graph``, include/camo_rg_features.h): ``image`` [H, W, 3] float in [0, 1], ``segments`` [H, W] integer
    superpixel labels (what ``slic`` returned, :144), ``edges_canny`` [H, W] bool (what ``canny`` returned, :152; ``None``: computed
    from ``image`` on the device by ``canny_edges``) ->
    (RegionGraphData on the device, region_map int32 [labels] = new index of each label or -1).  Regions are renumbered in
    increasing label order with empty labels dropped; edges come sorted by (i, j) with each followed by its reverse (the
    reference's order is networkx's iteration order: a permutation).  PARITY UNPINNED, see the header."""
    dev = torch.device(device)
    img = torch.as_tensor(image).to(device=dev, dtype=torch.float32).contiguous()
    seg = torch.as_tensor(segments).to(device=dev, dtype=torch.int32).contiguous()
    _lib.require_device(img, "image")
    if edges_canny is None:
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"need image [H, W, 3], got {tuple(img.shape)}")
        edges_canny = canny_edges(img)
    can = torch.as_tensor(edges_canny).to(device=dev).to(torch.uint8).contiguous()
    if img.dim() != 3 or img.shape[2] != 3 or seg.shape != img.shape[:2] or can.shape != img.shape[:2]:
        raise ValueError(f"need image [H, W, 3], segments [H, W], edges_canny [H, W]; got {tuple(img.shape)}, {tuple(seg.shape)}, {tuple(can.shape)}")
    H, W = seg.shape
    lo, hi = int(seg.min()), int(seg.max())
    if lo < 0 or hi >= _lib.RG_MAX_LABELS:
        raise ValueError(f"segment labels must lie in [0, {_lib.RG_MAX_LABELS}), got [{lo}, {hi}]")
    n_labels = hi + 1
    cap = int(edge_capacity) if edge_capacity else 16 * n_labels        # (a planar adjacency has < 3 n pairs; 8-connectivity adds corner contacts)
    while True:
        ws, nbytes = workspace("camo_rg_graph_workspace_bytes", n_labels, device=dev)
        x = torch.empty(n_labels, 15, dtype=torch.float32, device=dev)
        rmap = torch.empty(n_labels, dtype=torch.int32, device=dev)
        ei = torch.empty(2, cap, dtype=torch.int64, device=dev)
        ea = torch.empty(cap, dtype=torch.float32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        call("camo_rg_region_graph", dev, _ptr(img), _ptr(seg), _ptr(can), H, W, n_labels, _ptr(ws), nbytes, _ptr(x), _ptr(rmap), _ptr(ei),
             _ptr(ea), cap, _ptr(counts), _stream_ptr(dev))
        n, e = (int(v) for v in counts.tolist())                         # (the one synchronisation: the sizes of what was built)
        if e <= cap:
            break
        cap = e                                                          # the library reported the capacity needed: once more
    return RegionGraphData(x[:n], ei[:, :e], ea[:e].unsqueeze(1)), rmap


def create_region_graphs_from_segments(images, segments, edges_canny=None, device="cuda", label_bound=None, edge_capacity=None):
    """``create_region_graph_from_segments`` for a batch in one library call (``camo_rg_region_graph_batch``,
    include/camo_rg_batch.h): ``images`` [N, H, W, 3] float in [0, 1], ``segments`` [N, H, W] integer labels, ``edges_canny``
    [N, H, W] bool (``None``: one batched ``canny_edges`` call) -> (RegionGraphBatch on the device, region_map int32
    [N, label_bound] = index of each label within its image or -1).  Per image the graph is the single-image function's, up to
    the arithmetic: the sums are integers here (the header derives the bounds), so the result does not depend on the order the
    additions arrive in -- two calls give the same bytes and a batch the bytes of its images one by one.  ``label_bound``: every label
    must lie in [0, label_bound); ``None`` reads ``segments.max()`` back (one synchronisation more).  After the launch ONE
    device -> host copy brings the offsets and the status; a label out of range raises ``ValueError``, more edges than
    ``edge_capacity`` (default 16 N label_bound) run the call once more with the capacity it reported."""
    dev = torch.device(device)
    img, seg = _as_tensor(images, dev), _as_tensor(segments, dev)
    can = None if edges_canny is None else _as_tensor(edges_canny, dev)
    if img.dim() != 4 or img.shape[3] != 3 or img.numel() == 0 or seg.shape != img.shape[:3] or (can is not None and can.shape != img.shape[:3]):
        raise ValueError(f"need images [N, H, W, 3], segments [N, H, W], edges_canny [N, H, W]; got {tuple(img.shape)}, {tuple(seg.shape)}"
                         + ("" if can is None else f", {tuple(can.shape)}"))
    _lib.require_device(img, "images")
    dev = img.device
    img = img.to(torch.float32).contiguous()
    seg = seg.to(device=dev, dtype=torch.int32).contiguous()
    if can is None:
        can = canny_edges(img)
    can = can.to(device=dev).to(torch.uint8).contiguous()
    N, H, W = seg.shape
    if label_bound is None:
        label_bound = max(int(seg.max()), 0) + 1                          # (a negative label is the range check's, on the device)
    label_bound = int(label_bound)
    if label_bound < 1 or label_bound > _lib.RG_MAX_LABELS:
        raise ValueError(f"label_bound must lie in [1, {_lib.RG_MAX_LABELS}], got {label_bound}")
    nodes = N * label_bound
    cap = int(edge_capacity) if edge_capacity else 16 * nodes             # (a planar adjacency has < 3 n pairs; 8-connectivity adds corner contacts)
    ws, nbytes = workspace("camo_rg_batch_workspace_bytes", N, H, W, label_bound, device=dev)
    x = torch.empty(nodes, 15, dtype=torch.float32, device=dev)
    rmap = torch.empty(N, label_bound, dtype=torch.int32, device=dev)
    batch = torch.empty(nodes, dtype=torch.int32, device=dev)
    sizes = torch.empty(2 * (N + 1) + 2, dtype=torch.int32, device=dev)   # node_off, edge_off, status: one copy brings all three
    node_off, edge_off, status = sizes[:N + 1], sizes[N + 1:2 * (N + 1)], sizes[2 * (N + 1):]
    while True:
        ei = torch.empty(2, cap, dtype=torch.int64, device=dev)
        ea = torch.empty(cap, dtype=torch.float32, device=dev)
        call("camo_rg_region_graph_batch", dev, _ptr(img), _ptr(seg), _ptr(can), N, H, W, label_bound, _ptr(ws), nbytes, _ptr(x), nodes,
             _ptr(rmap), _ptr(ei), _ptr(ea), cap, _ptr(node_off), _ptr(edge_off), _ptr(batch), _ptr(status), _stream_ptr(dev))
        host = sizes.tolist()                                             # (the one synchronisation: the sizes of what was built)
        no, eo, (bad, e) = host[:N + 1], host[N + 1:2 * (N + 1)], host[2 * (N + 1):]
        if bad:
            raise ValueError(f"{bad} pixel{'s' if bad != 1 else ''} with a segment label outside [0, {label_bound})")
        if e <= cap:
            break
        cap = e                                                           # the library reported the capacity needed: once more
    n = no[N]
    return RegionGraphBatch(x[:n], ei[:, :e], ea[:e].unsqueeze(1), batch[:n], no, eo), rmap


def slic_label_bound(H, W, n_segments):
    """A bound on ``slic_segments``' labels that needs no look at them: labels < bound.  The connectivity step (include/camo_slic.h
    step 8) gives a new label only to a component of at least ``min_size = int(0.5 H W / K)`` pixels (K centroids,
    ``camo_slic_grid``), the components are disjoint, and labels start at 1 with 0 for pixels that adopt none: at most
    ``H W // max(min_size, 1)`` labels above 0.  Capped at ``RG_MAX_LABELS``; the device-side range check covers the rest."""
    out = (C.c_int32 * 5)()
    _lib.check(_lib.lib().camo_slic_grid(int(H), int(W), int(n_segments), out), "camo_slic_grid")
    min_size = int(0.5 * H * W / out[0])
    return min(H * W // max(min_size, 1) + 2, _lib.RG_MAX_LABELS)


def region_graphs_from_images(images, n_segments=500, device="cuda"):
    """``region_graph_from_image`` for a batch: ``slic_segments`` on ``images`` [N, H, W, 3] float in [0, 1], then
    ``create_region_graphs_from_segments`` (one batched Canny call inside) with ``slic_label_bound`` as the label bound, so the
    only synchronisation is the sizes read-back.  Returns (RegionGraphBatch on the device, segments int32 [N, H, W] on the device)."""
    img, _ = _image_batch(_as_tensor(images, device))
    _lib.require_device(img, "images")
    segments = slic_segments(img, n_segments)
    graphs, _ = create_region_graphs_from_segments(img, segments, device=img.device, label_bound=slic_label_bound(img.shape[1], img.shape[2], n_segments))
    return graphs, segments


def slic_segments(images, n_segments=500, compactness=10.0, sigma=1.0, device="cuda", return_counts=False):
    """``skimage.segmentation.slic((image * 255).astype(np.uint8), n_segments, compactness=10, sigma=1)`` of the reference
    (extract_rg_embeddings.py:143-144, the quantisation included) on the device (``camo_slic``, include/camo_slic.h): ``images``
    [H, W, 3] or [N, H, W, 3] float in [0, 1] -> int32 labels [H, W] or [N, H, W] on the device; with ``return_counts`` also int32
    [N, 2] ([2] for one image) = (largest label + 1, components of max_size pixels or more, which the device leaves whole).  A tensor
    is used where it is (``device`` places other inputs) and must be on a HIP device.  PARITY UNPINNED, see the header."""
    img = _as_tensor(images, device)
    _lib.require_device(img, "images")
    img, single = _image_batch(img, single_ok=True)
    dev = img.device
    N, H, W = img.shape[:3]
    ws, nbytes = workspace("camo_slic_workspace_bytes", N, H, W, int(n_segments), device=dev)
    labels = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    counts = torch.empty(N, 2, dtype=torch.int32, device=dev)
    call("camo_slic", dev, _ptr(img), N, H, W, int(n_segments), float(compactness), float(sigma), _ptr(ws), nbytes, _ptr(labels), _ptr(counts),
         _stream_ptr(dev))
    if single:
        labels, counts = labels[0], counts[0]
    return (labels, counts) if return_counts else labels


def region_graph_from_image(image, n_segments=500, device="cuda"):
    """``create_region_graph(image, n_segments)`` of the reference (extract_rg_embeddings.py:138) with nothing on the host:
    ``slic_segments`` then ``create_region_graph_from_segments`` (which computes the Canny edge map on the device).  ``image``
    [H, W, 3] float in [0, 1].  Returns (RegionGraphData on the device, segments int32 [H, W] on the device)."""
    img = _as_tensor(image, device)
    _lib.require_device(img, "image")
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"need image [H, W, 3], got {tuple(img.shape)}")
    img = img.to(torch.float32).contiguous()
    segments = slic_segments(img, n_segments)
    data, _ = create_region_graph_from_segments(img, segments, device=img.device)
    return data, segments


def predict_from_image(multimodal_model, rg_model, image, kg_embeddings_dict, device, n_segments=500):
    """The reference's ``predict_single_image`` from the image on, with no host-side image processing: superpixels, edge map and
    region graph on the device (``region_graph_from_image``), then ``predict_from_region_graph`` (test_multimodal.py, which stays
    the reference's per-image surface unchanged).  ``image`` [H, W, 3] float in [0, 1].  Returns what that function returns."""
    from .test_multimodal import predict_from_region_graph
    graph_data, _ = region_graph_from_image(image, n_segments, device)
    return predict_from_region_graph(multimodal_model, rg_model, graph_data, kg_embeddings_dict, device)


def create_region_graph(image, n_segments=500, device="cuda"):
    """``create_region_graph(image, n_segments)`` of the reference (extract_rg_embeddings.py:138): slic and canny are
    skimage's and stay on the host when skimage is installed; everything after them runs on the device.  Returns
    (RegionGraphData, segments)."""
    try:
        from skimage import feature
        from skimage.segmentation import slic
    except ImportError as err:
        raise _lib.CamoError("create_region_graph needs scikit-image for slic / canny (models/region_graph/extract_rg_embeddings.py:144,152); "
                             "pass their results to create_region_graph_from_segments instead, or call region_graph_from_image, which "
                             "computes both on the device") from err
    import numpy as np
    image = np.asarray(image)
    segments = slic((image * 255).astype(np.uint8), n_segments=n_segments, compactness=10, sigma=1)       # :143-144
    gray = np.dot(image[..., :3], [0.2989, 0.5870, 0.1140])                                               # :151
    data, _ = create_region_graph_from_segments(image, segments, feature.canny(gray, sigma=2), device)  # :152
    return data, segments


class _GATParams(nn.Module):
    """Parameter container with torch_geometric.nn.GATConv's state_dict names (``lin.weight``; ``lin_src.weight`` of
    older releases is accepted on load)."""

    def __init__(self, in_channels, out_channels, heads):
        super().__init__()
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.xavier_uniform_(self.att_src); nn.init.xavier_uniform_(self.att_dst); nn.init.xavier_uniform_(self.lin.weight)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for old in ("lin_src.weight", "lin_l.weight"):
            if prefix + old in state_dict and prefix + "lin.weight" not in state_dict:
                state_dict[prefix + "lin.weight"] = state_dict.pop(prefix + old)
        for dup in ("lin_dst.weight", "lin_r.weight"):
            state_dict.pop(prefix + dup, None)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class _GCNParams(nn.Module):
    """Parameter container with torch_geometric.nn.GCNConv's state_dict names."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.xavier_uniform_(self.lin.weight)


PIECE = 64      # floats: every parameter starts on a 256-byte boundary of a flat buffer


def flat_layout(shapes):
    """The flat layout of tensors of ``shapes`` in order: ([(offset, numel), ...], total floats).  Every piece is rounded up to 64
    floats -- the layout ``RegionGraphGNN.loss_and_gradients_csr`` gives its gradients."""
    pieces, at = [], 0
    for shape in shapes:
        n = 1
        for d in shape:
            n *= int(d)
        pieces.append((at, n))
        at += -(-n // PIECE) * PIECE
    return pieces, at


def loss_figures(loss):
    """The 0-d views of the loss a training call returns: [4], or [6] with the pixel term (include/camo_rg_pixel_loss.h)."""
    out = {"loss": loss[0], "mask_loss": loss[1], "instance_loss": loss[2], "edge_loss": loss[3]}
    if loss.numel() == 6:
        out.update(pixel_loss=loss[4] + loss[5], wbce=loss[4], wiou=loss[5])
    return out


class RegionGraphGNN(nn.Module):
    def __init__(self, in_channels=15, hidden_channels=128, num_classes=2, heads=4):
        super().__init__()
        h = hidden_channels
        self.conv1 = _GATParams(in_channels, h, heads)
        self.bn1 = nn.BatchNorm1d(h)
        self.conv2 = _GCNParams(h, h); self.bn2 = nn.BatchNorm1d(h)
        self.conv3 = _GCNParams(h, h); self.bn3 = nn.BatchNorm1d(h)
        self.conv4 = _GCNParams(h, h); self.bn4 = nn.BatchNorm1d(h)
        self.fc_shared = nn.Linear(h, h)
        # node-classification heads (forward / node_probabilities, eval mode only)
        self.fc_mask_1 = nn.Linear(h, h // 2); self.fc_mask_2 = nn.Linear(h // 2, num_classes)
        self.fc_instance_1 = nn.Linear(h, h // 2); self.fc_instance_2 = nn.Linear(h // 2, num_classes)
        self.fc_edge_1 = nn.Linear(h, h // 2); self.fc_edge_2 = nn.Linear(h // 2, 1)
        self._dims = _lib.CamoRgDims(in_channels, h, heads)
        self.num_classes = num_classes

    def _abi_order(self):
        """The one list of what the library reads, in its order: (the embedding path's 28 tensors of include/camo_rg_gnn.h, the
        heads' 12 of include/camo_rg_detect.h).  The gradient table of include/camo_rg_train.h is the first list without the
        batch norms' running statistics -- buffers, not parameters -- followed by the second."""
        bn_all = lambda bn: [bn.weight, bn.bias, bn.running_mean, bn.running_var]  # noqa: E731
        embed = [self.conv1.att_src, self.conv1.att_dst, self.conv1.bias, self.conv1.lin.weight, *bn_all(self.bn1)]
        for conv, bn in ((self.conv2, self.bn2), (self.conv3, self.bn3), (self.conv4, self.bn4)):
            embed += [conv.bias, conv.lin.weight, *bn_all(bn)]
        embed += [self.fc_shared.weight, self.fc_shared.bias]
        heads = []
        for name in ("fc_mask", "fc_instance", "fc_edge"):
            for layer in (getattr(self, name + "_1"), getattr(self, name + "_2")):
                heads += [layer.weight, layer.bias]
        assert (len(embed), len(heads)) == (_lib.RG_NPARAMS, _lib.RGD_NPARAMS)
        return embed, heads

    @staticmethod
    def _pointer_table(t):
        for p in t:
            _lib.require_device(p, "RegionGraphGNN parameters")
        keep = [p.detach().to(torch.float32).contiguous() for p in t]
        tab = (C.c_void_p * len(keep))(*[p.data_ptr() for p in keep])
        return tab, keep

    def _param_table(self):
        return self._pointer_table(self._abi_order()[0])

    @torch.no_grad()
    def extract_node_embeddings(self, data=None, x=None, edge_index=None, edge_attr=None):
        """[num_nodes, hidden] node embeddings (eval-mode BatchNorm, no dropout), extract_rg_embeddings.py:94-122.
        ``data``: any object with ``x``, ``edge_index``, ``edge_attr`` (a torch_geometric ``Data`` / ``Batch``)."""
        if data is not None:
            x, edge_index = data.x, data.edge_index
            edge_attr = getattr(data, "edge_attr", None)
        _lib.require_device(x, "x")
        _lib.require_device(edge_index, "edge_index")
        if x.dim() != 2 or x.shape[1] != self._dims.in_channels:
            raise RuntimeError(f"x of shape {tuple(x.shape)} does not match in_channels {self._dims.in_channels}")
        n = x.shape[0]
        ew = None if edge_attr is None or edge_attr.numel() == 0 else edge_attr.reshape(-1)     # :98
        rowptr, col, w = build_target_csr_device(n, edge_index, ew)
        x = x.detach().to(torch.float32).contiguous()
        ws, nbytes = workspace("camo_rg_workspace_bytes", C.byref(self._dims), n, device=x.device)
        out = torch.empty(n, self._dims.hidden, dtype=torch.float32, device=x.device)
        tab, keep = self._param_table()
        rc = _lib.lib().camo_rg_node_embeddings(C.byref(self._dims), tab, _ptr(x), _ptr(rowptr), _ptr(col), _ptr(w), n, col.shape[0],
                                                _ptr(ws), nbytes, _ptr(out), _stream_ptr())
        _lib.check(rc, "camo_rg_node_embeddings")
        return out

    def extract_graph_embedding(self, data):
        """[num_graphs, hidden]: mean of the node embeddings per graph (global_mean_pool, extract_rg_embeddings.py:124-135).
        Not an input of the fusion model (the reference only stores it next to the node embeddings); the pooling is index
        plumbing on the device."""
        emb = self.extract_node_embeddings(data)
        batch = getattr(data, "batch", None)
        if batch is None:
            return emb.mean(dim=0, keepdim=True)
        g = getattr(data, "num_graphs", None)                              # (a RegionGraphBatch knows it: no read-back)
        if g is None:
            g = int(batch.max().item()) + 1
        out = torch.zeros(g, emb.shape[1], dtype=emb.dtype, device=emb.device).index_add_(0, batch.long(), emb)
        return out / torch.bincount(batch.long(), minlength=g).clamp(min=1).unsqueeze(1).to(emb.dtype)

    def _head_table(self):
        return self._pointer_table(self._abi_order()[1])

    @torch.no_grad()
    def node_heads(self, emb):
        """The three heads on node embeddings [n, hidden] in one launch (``camo_rg_node_heads``, include/camo_rg_detect.h) ->
        (logits [n, 2 num_classes + 1] = mask | instance | edge, probs [n, 3] = P(mask = 1), P(instance = 1), sigmoid(edge))."""
        _lib.require_device(emb, "emb")
        if emb.dim() != 2 or emb.shape[1] != self._dims.hidden or emb.shape[0] < 1:
            raise RuntimeError(f"emb of shape {tuple(emb.shape)} does not match hidden {self._dims.hidden}")
        emb = emb.detach().to(torch.float32).contiguous()
        n = emb.shape[0]
        logits = torch.empty(n, 2 * self.num_classes + 1, dtype=torch.float32, device=emb.device)
        probs = torch.empty(n, 3, dtype=torch.float32, device=emb.device)
        tab, keep = self._head_table()
        call("camo_rg_node_heads", emb.device, C.byref(self._dims), self.num_classes, tab, _ptr(emb), n, _ptr(logits), _ptr(probs),
             _stream_ptr(emb.device))
        return logits, probs

    def node_probabilities(self, data):
        """[n, 3] per node: P(mask = 1), P(instance = 1), sigmoid(edge logit) -- what the reference's detector paints
        (models/region_graph/test.py::detect_camouflage).  Eval-mode arithmetic whatever the module's mode."""
        return self.node_heads(self.extract_node_embeddings(data))[1]

    def trainable_parameters(self):
        """The 32 parameters ``loss_and_gradients`` writes a gradient for, in the order of the gradient table of
        include/camo_rg_train.h: the embedding path's 20 (``_param_table`` without the running statistics), then the heads' 12."""
        embed, heads = self._abi_order()
        # (the running statistics are the list's only buffers, every layer being affine; the assert holds the result to the table)
        t = [p for p in embed if isinstance(p, nn.Parameter)] + heads
        assert len(t) == _lib.RGT_NGRADS
        return t

    @torch.no_grad()
    def _batch_norms(self):
        return [self.bn1, self.bn2, self.bn3, self.bn4]

    def _running_table(self, dev):
        """The 8 running statistics as the table ``camo_rg_loss_backward_bn`` updates in place (bn1 mean, bn1 var .. bn4 var), and
        the modules' momentum."""
        mom = {bn.momentum for bn in self._batch_norms()}
        if len(mom) != 1:
            raise _lib.CamoError("batch-statistics batch norm on the MI355X path needs one momentum for the four BatchNorm1d")
        bufs = []
        for bn in self._batch_norms():
            for t in (bn.running_mean, bn.running_var):
                if t is None:
                    raise _lib.CamoError("update_running needs BatchNorm1d layers that track running statistics")
                _lib.require_device(t, "RegionGraphGNN running statistics")
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise _lib.CamoError("the running statistics must be contiguous fp32 buffers on the device of x: they are updated in place")
                bufs.append(t)
        return (C.c_void_p * 8)(*[t.data_ptr() for t in bufs]), bufs, float(mom.pop())

    @staticmethod
    def _dropout_rates(dropout):
        """``dropout`` (None, a float for all three classes, or a (p_conv, p_shared, p_head) triple) -> the triple as the fp32 values
        the library receives, or None when every rate is 0.  Each rate must be finite and in [0, 1): ``ValueError`` otherwise."""
        if dropout is None:
            return None
        try:
            rates = tuple(float(v) for v in dropout) if isinstance(dropout, (tuple, list)) else (float(dropout),) * 3
        except (TypeError, ValueError):
            raise ValueError(f"dropout must be a float or a (p_conv, p_shared, p_head) triple, got {dropout!r}") from None
        if len(rates) != 3:
            raise ValueError(f"dropout must be a float or a (p_conv, p_shared, p_head) triple, got {dropout!r}")
        rates = tuple(C.c_float(v).value for v in rates)                        # what the C ABI sees
        if any(not (0.0 <= v < 1.0) for v in rates):                            # (NaN and the infinities fail the comparison)
            raise ValueError(f"every dropout rate must be finite and in [0, 1), got {dropout!r}")
        return rates if any(v > 0.0 for v in rates) else None

    @staticmethod
    def _training_entry(batch_stats, rates, pixel):
        """The library entry ``loss_and_gradients_csr`` calls: ``rates`` as ``_dropout_rates`` returns them, ``pixel`` its argument.
        Each entry takes the arguments of the one before it and more; at neutral extras they give the same bytes, so only this
        function says which one runs."""
        if pixel is not None:
            return "camo_rg_loss_backward_pixel"                                # (with zero rates when there is no dropout)
        if rates is not None:
            return "camo_rg_loss_backward_drop"
        return "camo_rg_loss_backward_bn" if batch_stats else "camo_rg_loss_backward"

    @torch.no_grad()
    def loss_and_gradients_csr(self, x, csr, reversed_csr, mask_target, instance_target, edge_target, loss_weights=(1., 1., 1.), out=None,
                               batch_stats=False, update_running=True, stats_out=None, dropout=None, seed=0, pixel=None):
        """``loss_and_gradients`` on CSR arrays the caller built: ``csr`` = (rowptr, col, w) by target, ``reversed_csr`` the same
        for the graph with every edge turned round (both from ``build_target_csr_device``; they must hold the same edges).  One
        library call (``camo_rg_loss_backward``, include/camo_rg_train.h).  Returns (loss fp32 [4] = total, mask, instance, edge;
        list of 32 gradient tensors in ``trainable_parameters`` order, views of one buffer).  The result is a function of the
        arrays alone: two calls on the same arrays give the same bytes.  ``out``: a contiguous fp32 device buffer of exactly the
        flat layout's size (every piece rounded up to 64 floats) that receives the gradients instead of a new one; its padding is
        not written.

        ``batch_stats=True``: the four batch norms normalise by the statistics of this call's nodes (``camo_rg_loss_backward_bn``,
        include/camo_rg_train_bn.h) -- ``model.train()`` arithmetic, without dropout unless ``dropout`` is given; the four conv-bias gradients are then exactly
        +0.  With ``update_running`` the modules' ``running_mean`` / ``running_var`` are updated in place with the modules'
        ``momentum`` and ``num_batches_tracked`` goes up by one, on the device.  ``stats_out``: a contiguous fp32 device tensor
        [4, 2, hidden] that receives the batch mean and biased variance of each layer.  With the default ``batch_stats=False``
        neither of the two is looked at and nothing changes, whatever the module's mode.

        ``dropout``: a float (all three classes) or a triple (p_conv, p_shared, p_head) of rates in [0, 1) -- inverted dropout after the
        four conv blocks, after ``relu(fc_shared)`` and after the heads' first layers (``camo_rg_loss_backward_drop``,
        include/camo_rg_train_drop.h), in whichever batch-norm mode ``batch_stats`` selects; with ``batch_stats=True`` this is the whole
        of ``model.train()`` arithmetic.  The masks are a function of ``seed`` (a 64-bit integer), the site and the element index:
        the same seed on the same arrays gives the same bytes, so a caller that wants fresh masks passes a new seed per step.
        ``None``, 0 or all zeros: the calls above, unchanged.  A bad rate raises ``ValueError`` before any device work.

        ``pixel``: a tuple (node_w, node_offsets, radius, weight) adds ``weight`` times the structure loss on the painted mask
        (``camo_rg_loss_backward_pixel``, include/camo_rg_pixel_loss.h; needs ``num_classes == 2``): ``node_w`` int64 [n, 2] of
        ``rg_finetune.pixel_loss_weights`` with ``radius``, ``node_offsets`` the first node of every image (images + 1 integers, list or
        tensor).  In every batch-norm and dropout mode; the loss returned is then fp32 [6] = total, mask, instance, edge, mean
        weighted BCE, mean weighted IoU.  ``None``: the calls above, byte for byte."""
        rates = self._dropout_rates(dropout)
        if pixel is not None:
            node_w, node_off, radius, w_pixel = pixel
            radius, w_pixel = int(radius), C.c_float(float(w_pixel)).value
            if not (0 <= radius <= _lib.RGPL_MAX_RADIUS):
                raise ValueError(f"the pixel loss's radius must be in [0, {_lib.RGPL_MAX_RADIUS}], got {radius}")
            if not (0.0 <= w_pixel < float("inf")):                              # (NaN fails the comparison)
                raise ValueError(f"the pixel loss's weight must be finite and >= 0, got {pixel[3]!r}")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be in [0, 2^64), got {seed}")
        _lib.require_device(x, "x")
        if x.dim() != 2 or x.shape[1] != self._dims.in_channels or x.shape[0] < 1:
            raise RuntimeError(f"x of shape {tuple(x.shape)} does not match in_channels {self._dims.in_channels}")
        n, dev = x.shape[0], x.device
        x = x.detach().to(torch.float32).contiguous()
        graph = []
        for t, dt in zip(tuple(csr) + tuple(reversed_csr), (torch.int32, torch.int32, torch.float32) * 2):
            _lib.require_device(t, "csr")
            graph.append(t.to(dt).contiguous())
        rowptr, col, w, rrowptr, rcol, rw = graph
        E = col.shape[0]
        if rowptr.shape[0] != n + 1 or rrowptr.shape[0] != n + 1 or w.shape[0] != E or rcol.shape[0] != E or rw.shape[0] != E:
            raise RuntimeError("the two CSRs do not describe the same graph of x.shape[0] nodes")
        tg = []
        for t, dt, name in ((mask_target, torch.int32, "mask_target"), (instance_target, torch.int32, "instance_target"),
                            (edge_target, torch.float32, "edge_target")):
            _lib.require_device(t, name)
            t = t.detach().reshape(-1).to(dt).contiguous()
            if t.shape[0] != n:
                raise RuntimeError(f"{name} has {t.shape[0]} entries for {n} nodes")
            tg.append(t)
        wm, wi, we = (float(v) for v in loss_weights)
        if pixel is not None:
            _lib.require_device(node_w, "pixel node_w")
            if node_w.dtype != torch.int64 or tuple(node_w.shape) != (n, 2):
                raise RuntimeError(f"pixel node_w must be int64 [{n}, 2], got {node_w.dtype} {tuple(node_w.shape)}")
            node_w = node_w.to(dev).contiguous()
            node_off = (node_off.to(device=dev, dtype=torch.int32) if isinstance(node_off, torch.Tensor)
                        else torch.tensor(list(node_off), dtype=torch.int32, device=dev)).reshape(-1).contiguous()
            if node_off.numel() < 2:
                raise RuntimeError("pixel node_offsets must hold images + 1 >= 2 integers")
        if batch_stats:
            if any(bn.eps != 1e-5 for bn in self._batch_norms()):
                raise _lib.CamoError("batch-statistics batch norm on the MI355X path is built for eps = 1e-5 only")
            if any(bn.momentum is None for bn in self._batch_norms()):
                raise _lib.CamoError("batch-statistics batch norm on the MI355X path needs a float momentum (momentum=None, the "
                                     "cumulative average, is not built)")
            if n < 2:
                raise _lib.CamoError("batch-statistics batch norm needs at least 2 nodes")
            rtab, rkeep, momentum = self._running_table(dev) if update_running else (None, None, 0.0)
            if stats_out is not None:
                _lib.require_device(stats_out, "stats_out")
                if stats_out.dtype != torch.float32 or tuple(stats_out.shape) != (4, 2, self._dims.hidden) or not stats_out.is_contiguous() \
                        or stats_out.device != dev:
                    raise RuntimeError(f"stats_out must be a contiguous fp32 tensor [4, 2, {self._dims.hidden}] on {dev}")
        ws, nbytes = workspace("camo_rg_train_bn_workspace_bytes" if batch_stats else "camo_rg_train_workspace_bytes", C.byref(self._dims),
                               self.num_classes, n, E, device=dev)
        params = self.trainable_parameters()
        pieces, total = flat_layout([p.shape for p in params])
        if out is None:
            flat = torch.empty(total, dtype=torch.float32, device=dev)
        else:
            _lib.require_device(out, "out")
            if out.dtype != torch.float32 or out.dim() != 1 or out.numel() != total or not out.is_contiguous() or out.device != dev:
                raise RuntimeError(f"out must be a contiguous fp32 buffer of {total} floats on {dev}")
            flat = out
        grads = [flat[at:at + k].view(p.shape) for (at, k), p in zip(pieces, params)]
        loss = torch.empty(4 if pixel is None else 6, dtype=torch.float32, device=dev)
        tab, keep = self._param_table()
        htab, hkeep = self._head_table()
        gtab = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        # what every entry takes (and the stream, which goes last); then the batch-norm tail; then the dropout and pixel entries' own
        common = (C.byref(self._dims), self.num_classes, tab, htab, _ptr(x), _ptr(rowptr), _ptr(col), _ptr(w), _ptr(rrowptr), _ptr(rcol),
                  _ptr(rw), n, E, _ptr(tg[0]), _ptr(tg[1]), _ptr(tg[2]), wm, wi, we, _ptr(ws), nbytes, _ptr(loss), gtab)
        name = self._training_entry(batch_stats, rates, pixel)
        tail = ()
        if name != "camo_rg_loss_backward":
            tail = (momentum, rtab, None if stats_out is None else _ptr(stats_out)) if batch_stats else (0.0, None, None)
        if name in ("camo_rg_loss_backward_drop", "camo_rg_loss_backward_pixel"):
            tail += (1 if batch_stats else 0, *(rates or (0.0, 0.0, 0.0)), seed)
        if name == "camo_rg_loss_backward_pixel":
            tail += (_ptr(node_w), _ptr(node_off), node_off.numel() - 1, radius, w_pixel)
        call(name, dev, *common, *tail, _stream_ptr(dev))
        if batch_stats and update_running:
            for bn in self._batch_norms():
                if bn.num_batches_tracked is not None:
                    bn.num_batches_tracked.add_(1)
        return loss, grads

    @torch.no_grad()
    def loss_and_gradients(self, data, mask_target, instance_target, edge_target, loss_weights=(1., 1., 1.), accumulate=False, csr=None,
                           batch_stats=False, update_running=True, dropout=None, seed=0, pixel=None):
        """Loss on the three node heads and the gradient of every trainable parameter, with the BatchNorm layers on their running
        statistics and dropout off: eval-mode arithmetic (like ``node_probabilities``, whatever the module's mode) plus a backward --
        fine-tuning with frozen statistics (include/camo_rg_train.h).  ``data``: a ``RegionGraphData`` or ``RegionGraphBatch`` (the
        loss means then run over the whole block-diagonal graph).  Per node: ``mask_target`` / ``instance_target`` integer class or
        -1 to ignore the node, ``edge_target`` float in [0, 1] or negative to ignore it.
        ``loss = w_m CE(mask) + w_i CE(instance) + w_e BCEWithLogits(edge)``, each a mean over its non-ignored nodes (0 when there are
        none).  Sets ``.grad`` of the 32 ``trainable_parameters()`` (adds into an existing ``.grad`` with ``accumulate``); the running
        statistics are not touched, and any torch optimizer can step on the result.  Returns 0-d device tensors ``loss``,
        ``mask_loss``, ``instance_loss``, ``edge_loss``.  Both CSRs are built on the device and ONE library call does the rest; no
        host synchronisation.  ``csr``: the pair (CSR by target, CSR of the reversed graph) of an earlier
        ``build_target_csr_device`` of this graph, for a graph that is trained on again and again; the builder leaves a row's edges in
        no particular order, so only calls on the same pair are sure to add in the same order and give the same bytes.
        ``batch_stats=True``: batch norm on the statistics of the call's nodes, the running statistics updated in place unless
        ``update_running`` is false (see ``loss_and_gradients_csr``); a block-diagonal batch is one population.
        ``dropout`` / ``seed``: inverted dropout at the model's eight sites (see ``loss_and_gradients_csr``); the default is none.
        ``pixel``: (node_w, node_offsets, radius, weight) adds the structure loss on the painted mask (see ``loss_and_gradients_csr``);
        the returned dict then also carries ``pixel_loss`` (mean weighted BCE + mean weighted IoU), ``wbce`` and ``wiou``."""
        self._dropout_rates(dropout)                                             # a bad rate raises before the CSRs are built
        x, edge_index = data.x, data.edge_index
        edge_attr = getattr(data, "edge_attr", None)
        _lib.require_device(x, "x")
        _lib.require_device(edge_index, "edge_index")
        n = x.shape[0]
        ew = None if edge_attr is None or edge_attr.numel() == 0 else edge_attr.reshape(-1)
        if csr is None:
            csr = (build_target_csr_device(n, edge_index, ew), build_target_csr_device(n, edge_index.flip(0), ew))
        csr, rcsr = csr
        loss, grads = self.loss_and_gradients_csr(x, csr, rcsr, mask_target, instance_target, edge_target, loss_weights,
                                                  batch_stats=batch_stats, update_running=update_running, dropout=dropout, seed=seed, pixel=pixel)
        for p, g in zip(self.trainable_parameters(), grads):
            g = g.to(p.dtype)
            if accumulate and p.grad is not None:
                p.grad.add_(g)
            else:
                p.grad = g
        return loss_figures(loss)

    def forward(self, data):
        """Eval mode: (mask_logits [n, c], instance_logits [n, c], edge_logits [n, 1]), views of one tensor.  Training mode raises:
        a training-mode LOGITS entry (batch statistics and dropout without the loss and the backward) is not built -- training runs
        through ``loss_and_gradients``, which gives the loss and every gradient in one call, with the statistics frozen or with
        ``batch_stats=True`` and ``dropout=`` for the whole of ``model.train()`` arithmetic."""
        if self.training:
            raise _lib.CamoError("RegionGraphGNN.forward in training mode: a training mode logits entry is outside the MI355X path (a "
                                 "different feature from training itself); call .eval() for the node-classification heads, or use "
                                 "extract_node_embeddings().  To train, call loss_and_gradients(): the loss and gradients with the batch-norm "
                                 "statistics frozen, or with batch_stats=True and dropout=(p_conv, p_shared, p_head) as under model.train()")
        logits, _ = self.node_heads(self.extract_node_embeddings(data))
        c = self.num_classes
        return logits[:, :c], logits[:, c:2 * c], logits[:, 2 * c:]
