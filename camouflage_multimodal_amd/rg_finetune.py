"""Fine-tuning the region-graph detector from images and ground-truth masks on MI355X (include/camo_rg_targets.h).

What models/region_graph/train.py does around its forward and backward, with the batch-norm statistics frozen and dropout off (the
path of ``RegionGraphGNN.loss_and_gradients``): ``node_targets_from_masks`` turns ground-truth masks into one target per superpixel
for the three node heads (``camo_rg_node_targets``, three launches), ``prepare_finetune_batch`` builds everything a step reads from
a batch of images once (``prepare_finetune_batch_ragged``: from uint8 images of mixed sizes, through resize.py), and ``RegionGraphFineTuner`` holds the 32 trainable parameters in one flat buffer and takes a step as one
``camo_rg_loss_backward`` plus the two launches of the clip + AdamW pair of optim.py (``batch_norm="batch"`` and ``dropout=`` switch the
step to batch statistics and to dropout: include/camo_rg_train_bn.h, include/camo_rg_train_drop.h; ``pixel_loss=`` adds F3Net's structure
loss on the painted mask from ``pixel_loss_weights``, two launches over the ground truth: include/camo_rg_pixel_loss.h).  PARITY UNPINNED: the reference's CODDataset
cannot be read here, so the header's text defines the targets.  There is no CPU path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call
from .engine import _on
from .optim import AdamWStateMixin
from .region_graph import (PIECE, _as_tensor, _image_batch, build_target_csr_device, create_region_graphs_from_segments,  # noqa: F401
                           flat_layout, loss_figures, slic_label_bound, slic_segments)
from .pipeline import detect_camouflage_batch, detect_camouflage_ragged
from .augment import affine_rows, augment_batch
from .resize import _mask_list, _packed, _ragged, resize_batch
from .rg_detect import _offsets_tensor


def _mask_bytes(mask, name, shape, dev):
    """A uint8 [N, H, W] device mask (positive above 127) from uint8 or bool, as ``segmentation_counts`` takes them."""
    if mask is None:
        return None
    m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
    _lib.require_device(m, name)
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"need {name} [N, H, W] = {tuple(shape)}, got {tuple(m.shape)}")
    m = m.to(device=dev)
    return (m.to(torch.uint8) * 255 if m.dtype == torch.bool else m.to(torch.uint8)).contiguous()


@torch.no_grad()
def node_targets_from_masks(segments, region_map, node_offsets, gt_masks, instance_masks=None, edge_masks=None, band_permille=0,
                            edge_min_pixels=1, n_nodes=None):
    """One target per node of a block-diagonal batch of region graphs from ground-truth masks (``camo_rg_node_targets``,
    include/camo_rg_targets.h): ``segments`` [N, H, W] integer labels, ``region_map`` [N, label_bound] and ``node_offsets`` (N + 1
    integers, list or tensor) as ``create_region_graphs_from_segments`` returns them (what ``paint_regions`` takes; one image
    [H, W] with ``region_map`` [labels] is N = 1); ``gt_masks`` and the optional ``instance_masks`` / ``edge_masks`` [N, H, W] uint8
    (positive above 127) or bool.  Returns (mask_target int32 [n], instance_target int32 [n], edge_target fp32 [n], counts int32
    [n, 4] = pixels, mask-positive, instance-positive and edge pixels of every node) on the device, ready for
    ``loss_and_gradients``: a node is 1 when more than ``500 + band_permille`` thousandths of its pixels are positive, 0 at
    ``500 - band_permille`` or fewer, -1 (ignored) between; its edge target is 1 with ``edge_min_pixels`` edge pixels or more.
    Without ``instance_masks`` the mask stands in; without ``edge_masks`` the mask's boundary does.  Integer sums: two calls give
    the same bytes.  ``n`` is the last of ``node_offsets`` (a device tensor is read back for it unless ``n_nodes`` is given)."""
    _lib.require_device(segments, "segments")
    _lib.require_device(region_map, "region_map")
    dev = segments.device
    if segments.dim() == 2:
        segments, region_map = segments.unsqueeze(0), region_map.reshape(1, -1)
    if segments.dim() != 3 or region_map.dim() != 2 or region_map.shape[0] != segments.shape[0] or segments.numel() == 0 \
            or region_map.numel() == 0:
        raise ValueError(f"need segments [N, H, W] and region_map [N, label_bound]; got {tuple(segments.shape)}, {tuple(region_map.shape)}")
    N, H, W = segments.shape
    if n_nodes is None:
        n_nodes = int(node_offsets[-1])
    off = _offsets_tensor(node_offsets, dev)
    if off.numel() != N + 1:
        raise ValueError(f"node_offsets must hold N + 1 = {N + 1} integers, got {off.numel()}")
    gt = _mask_bytes(gt_masks, "gt_masks", (N, H, W), dev)
    if gt is None:
        raise ValueError("gt_masks is required")
    inst = _mask_bytes(instance_masks, "instance_masks", (N, H, W), dev)
    edge = _mask_bytes(edge_masks, "edge_masks", (N, H, W), dev)
    seg = segments.to(dtype=torch.int32).contiguous()
    rmap = region_map.to(device=dev, dtype=torch.int32).contiguous()
    n = int(n_nodes)
    counts = torch.empty(max(n, 0), 4, dtype=torch.int32, device=dev)
    mask_t = torch.empty(max(n, 0), dtype=torch.int32, device=dev)
    inst_t = torch.empty(max(n, 0), dtype=torch.int32, device=dev)
    edge_t = torch.empty(max(n, 0), dtype=torch.float32, device=dev)
    call("camo_rg_node_targets", dev, _ptr(seg), _ptr(rmap), _ptr(off), _ptr(gt), _ptr(inst), _ptr(edge), N, H, W, rmap.shape[1], n,
         int(band_permille), int(edge_min_pixels), _ptr(counts), _ptr(mask_t), _ptr(inst_t), _ptr(edge_t), _stream_ptr(dev))
    return mask_t, inst_t, edge_t, counts


@torch.no_grad()
def pixel_loss_weights(segments, region_map, node_offsets, gt_masks, radius=15, gain=5, n_nodes=None):
    """The two integer weights per node that turn F3Net's structure loss on the painted mask into a loss on the nodes
    (``camo_rg_pixel_weights``, include/camo_rg_pixel_loss.h, two launches): arguments as ``node_targets_from_masks`` takes them.
    With K = (2 radius + 1)^2 and S the sum of the ground truth over the K-window around a pixel (zero padding), a pixel weighs
    q = K + gain |S - K g|; returns int64 [n, 2] on the device = (sum q, sum q g) over every node's pixels, what
    ``loss_and_gradients(pixel=(node_w, node_offsets, radius, weight))`` takes.  Integer sums: two calls give the same bytes."""
    _lib.require_device(segments, "segments")
    _lib.require_device(region_map, "region_map")
    dev = segments.device
    if segments.dim() == 2:
        segments, region_map = segments.unsqueeze(0), region_map.reshape(1, -1)
    if segments.dim() != 3 or region_map.dim() != 2 or region_map.shape[0] != segments.shape[0] or segments.numel() == 0 \
            or region_map.numel() == 0:
        raise ValueError(f"need segments [N, H, W] and region_map [N, label_bound]; got {tuple(segments.shape)}, {tuple(region_map.shape)}")
    N, H, W = segments.shape
    if n_nodes is None:
        n_nodes = int(node_offsets[-1])
    off = _offsets_tensor(node_offsets, dev)
    if off.numel() != N + 1:
        raise ValueError(f"node_offsets must hold N + 1 = {N + 1} integers, got {off.numel()}")
    gt = _mask_bytes(gt_masks, "gt_masks", (N, H, W), dev)
    if gt is None:
        raise ValueError("gt_masks is required")
    seg = segments.to(dtype=torch.int32).contiguous()
    rmap = region_map.to(device=dev, dtype=torch.int32).contiguous()
    n = int(n_nodes)
    node_w = torch.empty(max(n, 0), 2, dtype=torch.int64, device=dev)
    call("camo_rg_pixel_weights", dev, _ptr(seg), _ptr(rmap), _ptr(off), _ptr(gt), N, H, W, rmap.shape[1], n, int(radius), int(gain),
         _ptr(node_w), _stream_ptr(dev))
    return node_w


def _pixel_options(pixel_loss):
    """``pixel_loss`` of ``prepare_finetune_batch`` -> None, or (radius, gain)."""
    if pixel_loss is None or pixel_loss is False:
        return None
    if pixel_loss is True:
        return 15, 5
    if not isinstance(pixel_loss, dict) or set(pixel_loss) - {"radius", "gain"}:
        raise ValueError(f'pixel_loss must be None, True or a dict with "radius" and / or "gain", got {pixel_loss!r}')
    return int(pixel_loss.get("radius", 15)), int(pixel_loss.get("gain", 5))


class FineTuneBatch:
    """What a fine-tuning step reads, built once and kept on the device: ``graphs`` (RegionGraphBatch), ``segments`` int32
    [N, H, W], ``region_map`` int32 [N, label_bound], ``mask_target`` / ``instance_target`` / ``edge_target`` / ``counts`` of
    ``node_targets_from_masks``, and ``csr`` / ``reversed_csr`` (by target, and of the graph with every edge turned round).
    With the pixel loss also ``pixel_weights`` (int64 [n, 2] of ``pixel_loss_weights``), ``node_offsets`` (int32 [N + 1] on the
    device) and ``pixel_radius``; ``None`` without."""

    def __init__(self, graphs, segments, region_map, mask_target, instance_target, edge_target, counts, csr, reversed_csr,
                 pixel_weights=None, node_offsets=None, pixel_radius=None):
        self.graphs, self.segments, self.region_map = graphs, segments, region_map
        self.mask_target, self.instance_target, self.edge_target, self.counts = mask_target, instance_target, edge_target, counts
        self.csr, self.reversed_csr = csr, reversed_csr
        self.pixel_weights, self.node_offsets, self.pixel_radius = pixel_weights, node_offsets, pixel_radius


@torch.no_grad()
def prepare_finetune_batch(images, gt_masks, instance_masks=None, edge_masks=None, n_segments=500, band_permille=0, device="cuda",
                           edge_min_pixels=1, pixel_loss=None):
    """``images`` [N, H, W, 3] float in [0, 1] and their ground-truth masks [N, H, W] -> ``FineTuneBatch``: superpixels, edge maps
    and region graphs on the device (region_graph.py), the node targets, and both CSRs built once with ``build_target_csr_device``,
    so that a resident dataset is trained on epoch after epoch through the ``csr=`` path of ``loss_and_gradients`` with nothing
    rebuilt.  The only host synchronisation is the sizes read-back of ``create_region_graphs_from_segments``.
    ``pixel_loss``: ``True`` or ``{"radius": .., "gain": ..}`` (15 and 5 when left out) also stores ``pixel_loss_weights`` of the
    masks, which a ``RegionGraphFineTuner`` with ``pixel_loss > 0`` needs."""
    pixel = _pixel_options(pixel_loss)
    img, _ = _image_batch(_as_tensor(images, device))
    _lib.require_device(img, "images")
    N, H, W = img.shape[:3]
    segments = slic_segments(img, n_segments)
    graphs, region_map = create_region_graphs_from_segments(img, segments, device=img.device, label_bound=slic_label_bound(H, W, n_segments))
    gt = _as_tensor(gt_masks, img.device)
    inst = None if instance_masks is None else _as_tensor(instance_masks, img.device)
    edge = None if edge_masks is None else _as_tensor(edge_masks, img.device)
    mask_t, inst_t, edge_t, counts = node_targets_from_masks(segments, region_map, graphs.node_offsets, gt, inst, edge, band_permille,
                                                             edge_min_pixels)
    n, ew = graphs.x.shape[0], graphs.edge_attr.reshape(-1)
    csr = build_target_csr_device(n, graphs.edge_index, ew)
    rcsr = build_target_csr_device(n, graphs.edge_index.flip(0), ew)
    if pixel is None:
        return FineTuneBatch(graphs, segments, region_map, mask_t, inst_t, edge_t, counts, csr, rcsr)
    node_w = pixel_loss_weights(segments, region_map, graphs.node_offsets, gt, pixel[0], pixel[1], n_nodes=n)
    return FineTuneBatch(graphs, segments, region_map, mask_t, inst_t, edge_t, counts, csr, rcsr, node_w,
                         _offsets_tensor(graphs.node_offsets, img.device), pixel[0])


@torch.no_grad()
def prepare_finetune_batch_ragged(images, gt_masks, instance_masks=None, edge_masks=None, size=(256, 256), crops=None, flips=None, augment=None, **kw):
    """``prepare_finetune_batch`` for uint8 images and masks of mixed sizes: the images are resized to ``size`` bilinear, every mask
    nearest, all with the same ``crops`` and ``flips`` (``random_resized_crops`` draws them), and the result goes to
    ``prepare_finetune_batch`` with ``**kw`` (n_segments, band_permille, device, edge_min_pixels, pixel_loss).
    ``augment`` -- a dict of ``augment.random_cod_augmentation``, in the place of ``crops`` and ``flips`` (giving both raises) -- adds
    its rotation and its four enhancement factors (include/camo_augment.h): the images go through ``augment_batch`` bilinear with the
    factors, every mask through the same maps nearest without them, what lies outside an image is 0.  ``augment=None`` (the
    default) is the path above, launch for launch."""
    if augment is not None and (crops is not None or flips is not None):
        raise ValueError("augment holds its own crops and flips: give crops and flips, or augment, not both")
    device = kw.get("device", "cuda")
    data, geo, C, _ = _ragged(images, device)
    if C != 3:
        raise ValueError(f"need images with 3 channels, got {C}")
    packed = _packed(data, geo, C)
    if augment is not None:
        rows = affine_rows(packed.sizes, size, augment["crops"], augment["flips"], augment["angles"], border="constant", fill=0)
        img = augment_batch(packed, size, rows, augment.get("factors"), "bilinear")
    else:
        img = resize_batch(packed, size, "bilinear", crops, flips)
    kw["device"] = img.device

    def small(masks, name):
        if masks is None:
            return None
        m = _mask_list(masks, len(packed), name, img.device)
        if m.sizes != packed.sizes:
            raise ValueError(f"every one of {name} must have its image's size")
        if augment is not None:
            return augment_batch(m, size, rows, None, "nearest", out_dtype=torch.uint8)
        return resize_batch(m, size, "nearest", crops, flips, out_dtype=torch.uint8)

    return prepare_finetune_batch(img, small(gt_masks, "gt_masks"), small(instance_masks, "instance_masks"), small(edge_masks, "edge_masks"),
                                  **kw)


class RegionGraphFineTuner(AdamWStateMixin):
    """Clip + AdamW fine-tuning of a ``RegionGraphGNN`` with its batch-norm statistics frozen.  At construction the model's 32
    ``trainable_parameters()`` become views of ONE flat fp32 buffer (``flat_layout``: pieces rounded up to 64 floats, padding zero),
    so ``state_dict``, ``load_state_dict`` and every method of the model keep working; the flat gradient, first- and second-moment
    buffers are allocated once.  ``step`` is ``camo_rg_loss_backward`` into the flat gradient buffer, then ``camo_grad_sumsq`` and
    ``camo_clip_adamw`` over the flat buffers: ``torch.nn.utils.clip_grad_norm_(max_norm)`` followed by ``torch.optim.AdamW`` on the
    32 parameters, with no host synchronisation.  The running statistics are buffers of the model and are never written --
    unless ``batch_norm="batch"``: a step is then ``camo_rg_loss_backward_bn`` (batch statistics, include/camo_rg_train_bn.h), which
    updates the four layers' running statistics in place, the only thing outside the flat buffers that a step writes.
    ``batch_norm="frozen"`` (the default) is the frozen path; any other value raises.
    ``dropout`` (a float or a (p_conv, p_shared, p_head) triple; ``None``, the default, is none) makes a step
    ``camo_rg_loss_backward_drop`` (include/camo_rg_train_drop.h) in the chosen batch-norm mode; the step that follows ``step_count``
    finished steps draws its masks from seed ``seed + step_count`` -- a host counter, no synchronisation -- and ``step_count`` is what
    ``state_dict`` / ``load_state_dict`` already carry, so a resumed run continues the mask sequence.
    ``pixel_loss`` (a weight, 0.0 = off and no launch more) adds that many times F3Net's structure loss on the painted mask to the
    loss of every step (``camo_rg_loss_backward_pixel``, include/camo_rg_pixel_loss.h) in whichever mode the other arguments choose;
    ``step`` then needs a batch prepared with ``pixel_loss=``, which ``step_from_images`` and ``step_from_ragged`` do with
    ``pixel_radius`` and ``pixel_gain``.  ``loss_weights=(0, 1, 1)`` beside it trains the mask head on pixels alone."""

    def __init__(self, rg_model, lr=1e-4, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, loss_weights=(1.0, 1.0, 1.0),
                 batch_norm="frozen", dropout=None, seed=0, pixel_loss=0.0, pixel_radius=15, pixel_gain=5):
        if batch_norm not in ("frozen", "batch"):
            raise ValueError(f'batch_norm must be "frozen" or "batch", got {batch_norm!r}')
        self.pixel_loss, self.pixel_radius, self.pixel_gain = float(pixel_loss), int(pixel_radius), int(pixel_gain)
        if not (0.0 <= self.pixel_loss < float("inf")):
            raise ValueError(f"pixel_loss must be finite and >= 0, got {pixel_loss!r}")
        if not (0 <= self.pixel_radius <= _lib.RGPL_MAX_RADIUS and 0 <= self.pixel_gain <= _lib.RGPL_MAX_GAIN):
            raise ValueError(f"pixel_radius must be in [0, {_lib.RGPL_MAX_RADIUS}] and pixel_gain in [0, {_lib.RGPL_MAX_GAIN}], got "
                             f"{pixel_radius!r}, {pixel_gain!r}")
        self.batch_norm = batch_norm
        rg_model._dropout_rates(dropout)                            # a bad rate raises here, not at the first step
        self.dropout, self.seed = dropout, int(seed)
        self.model = rg_model
        self.base_lr = self.lr = float(lr)
        self.weight_decay, self.betas, self.eps, self.max_norm = float(weight_decay), tuple(betas), float(eps), float(max_norm)
        self.loss_weights = tuple(float(w) for w in loss_weights)
        self.step_count = 0
        params = rg_model.trainable_parameters()
        names = {id(p): k for k, p in rg_model.named_parameters()}
        dev = params[0].device
        if any(p.device != dev or p.dtype != torch.float32 for p in params):
            raise ValueError("RegionGraphFineTuner needs every trainable parameter in fp32 on one device")
        pieces, total = flat_layout([p.shape for p in params])
        self.flat_params = torch.zeros(total, dtype=torch.float32, device=dev)
        self._entries = []                                          # (parameter, name, offset, numel, shape): the layout of engine.py
        with torch.no_grad():
            for p, (o, n) in zip(params, pieces):
                view = self.flat_params[o:o + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
                self._entries.append((p, names[id(p)], o, n, tuple(p.shape)))
        self.flat_grads = torch.zeros_like(self.flat_params)
        self.grads = [self.flat_grads[o:o + n].view(shape) for _, _, o, n, shape in self._entries]
        self._m = torch.zeros_like(self.flat_params)
        self._v = torch.zeros_like(self.flat_params)
        self._sumsq = torch.zeros(_lib.SUMSQ_FLOATS, dtype=torch.float32, device=dev)

    def _layout(self):
        return self._entries

    def _state(self):
        return self._m, self._v, self._sumsq

    def _check_resident(self):
        base, dev = self.flat_params.data_ptr(), self.flat_params.device
        for p, name, o, n, shape in self._entries:
            if p.device != dev or p.data_ptr() != base + 4 * o or tuple(p.shape) != shape or not p.is_contiguous():
                raise _lib.CamoError(f"parameter {name} no longer lives in the fine-tuner's flat buffer (the model was moved or its "
                                     "parameters were replaced after the tuner was built): build a new RegionGraphFineTuner for the model "
                                     "as it is now; this one would train a copy")

    @torch.no_grad()
    def step(self, batch):
        """One clip + AdamW step on a ``FineTuneBatch``.  Returns 0-d device tensors ``loss``, ``mask_loss``, ``instance_loss``,
        ``edge_loss`` of the parameters BEFORE the update -- with ``pixel_loss > 0`` also ``pixel_loss``, ``wbce`` and ``wiou``.  No
        host synchronisation; the gradient buffer is the tuner's own."""
        _lib.require_device(self.flat_params, "RegionGraphFineTuner parameters")
        self._check_resident()
        pixel = None
        if self.pixel_loss > 0.0:
            if getattr(batch, "pixel_weights", None) is None or batch.node_offsets is None or batch.pixel_radius is None:
                raise ValueError("pixel_loss > 0 needs a batch that carries pixel_weights, node_offsets and pixel_radius: prepare it with "
                                 "prepare_finetune_batch(..., pixel_loss=True)")
            pixel = (batch.pixel_weights, batch.node_offsets, batch.pixel_radius, self.pixel_loss)
        loss, _ = self.model.loss_and_gradients_csr(batch.graphs.x, batch.csr, batch.reversed_csr, batch.mask_target, batch.instance_target,
                                                    batch.edge_target, self.loss_weights, out=self.flat_grads,
                                                    batch_stats=self.batch_norm == "batch", dropout=self.dropout,
                                                    seed=(self.seed + self.step_count) & 0xFFFFFFFFFFFFFFFF, pixel=pixel)
        p, g, (m, v, ss) = self.flat_params, self.flat_grads, self._state()
        self.step_count += 1
        L = _lib.lib()
        with _on(p.device):
            st = _stream_ptr(p.device)
            _lib.check(L.camo_grad_sumsq(_ptr(g), g.numel(), _ptr(ss), st), "camo_grad_sumsq")
            _lib.check(L.camo_clip_adamw(_ptr(p), _ptr(g), _ptr(m), _ptr(v), g.numel(), _ptr(ss), self.max_norm, self.lr, self.betas[0],
                                         self.betas[1], self.eps, self.weight_decay, self.step_count, 0, st), "camo_clip_adamw")
        return loss_figures(loss)

    def _pixel_options(self):
        return {"radius": self.pixel_radius, "gain": self.pixel_gain} if self.pixel_loss > 0.0 else None

    def step_from_images(self, images, gt_masks, instance_masks=None, edge_masks=None, n_segments=500, band_permille=0, edge_min_pixels=1):
        """``prepare_finetune_batch`` on the tuner's device (with the pixel weights when ``pixel_loss > 0``), then ``step``."""
        _lib.require_device(self.flat_params, "RegionGraphFineTuner parameters")
        return self.step(prepare_finetune_batch(images, gt_masks, instance_masks, edge_masks, n_segments, band_permille,
                                                self.flat_params.device, edge_min_pixels, self._pixel_options()))

    @staticmethod
    def _evaluation(out, cod_metrics, instances, match, native=False, boundary=None, split=None):
        match = None if match is False else match
        if not (instances or match is not None):
            return {"metrics": out["metrics"], "cod_metrics": out["cod_metrics"]} if cod_metrics else out["metrics"]
        res = {"metrics": out["metrics"], "instances": out["instances_native" if native else "instances"]}
        if split is not None and split is not False:
            res["split_instances"] = out["split_instances_native" if native else "split_instances"]
        if cod_metrics:
            res["cod_metrics"] = out["cod_metrics"]
        if match is not None:
            res["instance_match"] = out["instance_match"]
        if boundary is not None and boundary is not False:
            res["boundary_match"] = out["boundary_match"]
            if "boundary_iou" in out:
                res["boundary_iou"] = out["boundary_iou"]
        return res

    def evaluate(self, images, gt_masks, n_segments=500, threshold=0.5, cod_metrics=False, instances=False, match=None, min_area=0,
                 fill_holes=False, connectivity=8, *, boundary=None, split=None):
        """``detect_camouflage_batch``'s metrics of the model as it is now: a list of ``segmentation_metrics`` dicts, one per image.
        With ``cod_metrics=True`` a dict instead: that list under "metrics" and, under "cod_metrics", the list of the benchmark
        measures (S-alpha, E-phi, F-beta, MAE on the 8-bit map, ``wf``) of ``seg_measures.cod_metrics``.  With ``instances=True``
        (``detect_camouflage_batch``'s, with ``min_area``, ``fill_holes``, ``connectivity``) a dict that also carries "instances"
        and, with ``match`` (``True`` or ``detect_camouflage_batch``'s dict), "instance_match": the records of the instances
        matched to the ground-truth ones; with ``boundary`` (``detect_camouflage_batch``'s; needs ``match``) also "boundary_match",
        the records under min(mask IoU, boundary IoU), and "boundary_iou" of the thresholded masks.  With ``split``
        (``detect_camouflage_batch``'s: ``True`` or a dict, ``{"growth": "geodesic"}`` for connected parts, ``{"merge": (4, 5)}`` to
        join the parts again across their high passes; needs ``instances=True``)
        also "split_instances", the records of the instances split at their necks, and "instance_match" and "boundary_match" are
        then those of the split instances, as in the pipeline.  ``split=None``: nothing changes."""
        _lib.require_device(self.flat_params, "RegionGraphFineTuner parameters")
        split = False if split is None else split
        out = detect_camouflage_batch(self.model, images, gt_masks, n_segments, threshold, self.flat_params.device, cod_metrics, instances, min_area,
                                      fill_holes, connectivity, match=match, boundary=boundary, split=split)
        return self._evaluation(out, cod_metrics, instances, match, boundary=boundary, split=split)

    def step_from_ragged(self, images, gt_masks, instance_masks=None, edge_masks=None, size=(256, 256), crops=None, flips=None, n_segments=500,
                         band_permille=0, edge_min_pixels=1, augment=None):
        """``prepare_finetune_batch_ragged`` (uint8 images and masks of mixed sizes, resized to ``size`` on the tuner's
        device with a crop box and a flip per image -- or with ``augment``, a dict of ``augment.random_cod_augmentation``: crop,
        flip, rotation and the four enhancements), then ``step``."""
        _lib.require_device(self.flat_params, "RegionGraphFineTuner parameters")
        return self.step(prepare_finetune_batch_ragged(images, gt_masks, instance_masks, edge_masks, size, crops, flips, augment, n_segments=n_segments,
                                                       band_permille=band_permille, device=self.flat_params.device,
                                                       edge_min_pixels=edge_min_pixels, pixel_loss=self._pixel_options()))

    def evaluate_ragged(self, images, gt_masks, size=(256, 256), n_segments=500, threshold=0.5, cod_metrics=False, evaluate_at="native",
                        instances=False, match=None, min_area=0, fill_holes=False, connectivity=8, *, boundary=None, split=None):
        """``evaluate`` for uint8 images and masks of mixed sizes (``detect_camouflage_ragged`` of pipeline.py): the metrics are taken
        against every mask at its own size, or at ``size`` with ``evaluate_at="resized"``.  Same return as ``evaluate``; the
        instances and their matches -- ``boundary``'s too -- are those of the native-size maps, and with ``split`` (``evaluate``'s)
        "split_instances" holds the native-size records ("split_instances_native" of the pipeline)."""
        _lib.require_device(self.flat_params, "RegionGraphFineTuner parameters")
        split = False if split is None else split
        out = detect_camouflage_ragged(self.model, images, gt_masks, size, n_segments, threshold, self.flat_params.device, cod_metrics, evaluate_at,
                                       instances, min_area, fill_holes, connectivity, match=match, boundary=boundary, split=split)
        return self._evaluation(out, cod_metrics, instances, match, native=True, boundary=boundary, split=split)
