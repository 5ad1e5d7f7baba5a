"""Node targets from ground-truth masks (include/camo_rg_targets.h) against tests/rg_targets_ref.py.

PARITY UNPINNED (the reference's CODDataset cannot be read here): the header is the definition, the numpy restatement the checker.
All the arithmetic is integer, so every GPU test compares every element of the four outputs for EXACT equality; there is no
tolerance anywhere in this file.  The CPU tests hold the header to the binding, the library's argument checks to the header, and the
restatement to properties it must have whatever the kernel does.
"""
import os

import numpy as np
import pytest
import torch

import rg_targets_ref as TG
from conftest import ROOT

E_ARG = -1


def _blobs(rs, N, H, W, k=3):
    """uint8 [N, H, W]: a few random discs per image, bytes 0 / 255 with some 127 / 128 sprinkled over both sides of the threshold."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        for _ in range(k):
            cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(3, max(4, min(H, W) / 3))
            out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
    odd = rs.uniform(size=out.shape) < 0.05
    out[odd] = np.where(out[odd] > 127, 128, 127).astype(np.uint8)
    return out


def _blocks(N, H, W, b):
    """int32 [N, H, W]: square blocks of side b, labelled row by row."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.broadcast_to(((yy // b) * (-(-W // b)) + xx // b).astype(np.int32), (N, H, W)).copy()


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_header_symbols_binding_and_abi_version():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_rg_targets.h")).read()
    assert _lib.symbols("camo_rg_targets.h") == ("camo_rg_node_targets",)
    assert "PARITY UNPINNED" in hdr and "train.py" in hdr and "THREE launches" in hdr and "No workspace" in hdr
    assert _lib.ABI_VERSION == 13 and "#define CAMO_ABI_VERSION 13" in open(os.path.join(ROOT, "include", "camo_fusion.h")).read()
    assert _lib.lib().camo_abi_version() == 13
    assert "camo_rg_targets.h" in open(os.path.join(ROOT, "include", "camo_rg_train.h")).read()


def test_argument_checks_match_the_header():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    fake = 0x1000                                    # never dereferenced: every check runs on the host before any launch
    names = ("segments", "region_map", "node_off", "gt_mask", "gt_instance", "gt_edge", "counts", "mask_t", "inst_t", "edge_t")

    def call(N=2, H=70, W=33, label_bound=64, n_nodes=50, band=0, emin=1, null=()):
        p = {k: (None if k in null else fake) for k in names}
        rc = L.camo_rg_node_targets(p["segments"], p["region_map"], p["node_off"], p["gt_mask"], p["gt_instance"], p["gt_edge"], N, H, W,
                                    label_bound, n_nodes, band, emin, p["counts"], p["mask_t"], p["inst_t"], p["edge_t"], None)
        return rc, L.camo_last_error()

    for kw, word in ((dict(N=0), b"N"), (dict(H=0), b"H"), (dict(W=-1), b"W"), (dict(label_bound=0), b"label_bound"),
                     (dict(label_bound=4097), b"label_bound"), (dict(n_nodes=0), b"n_nodes"),
                     (dict(N=1, H=8193, W=8192), b"CAMO_RGB_MAX_IMAGE_PIXELS"), (dict(N=3, H=8192, W=8192), b"CAMO_RGB_MAX_PIXELS"),
                     (dict(band=-1), b"band_permille"), (dict(band=500), b"band_permille"), (dict(emin=0), b"edge_min_pixels")):
        rc, msg = call(**kw)
        assert rc == E_ARG and word in msg, (kw, rc, msg)
    for name in ("segments", "region_map", "node_off", "gt_mask", "counts", "mask_t", "inst_t", "edge_t"):
        rc, msg = call(null=(name, "gt_instance", "gt_edge"))      # (the two optional masks null as well: not what is refused)
        assert rc == E_ARG and name.encode() in msg, (name, rc, msg)


def test_cpu_tensors_raise():
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN, node_targets_from_masks
    from camouflage_multimodal_amd._lib import CamoError
    seg = torch.zeros(1, 8, 8, dtype=torch.int32)
    with pytest.raises(CamoError):
        node_targets_from_masks(seg, torch.zeros(1, 1, dtype=torch.int32), [0, 1], torch.zeros(1, 8, 8, dtype=torch.uint8))
    tuner = RegionGraphFineTuner(RegionGraphGNN(hidden_channels=32, heads=2))
    with pytest.raises(CamoError):
        tuner.step(None)
    with pytest.raises(CamoError):
        tuner.step_from_images(torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(CamoError):
        tuner.evaluate(torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_reference_pixel_counts_sum_to_the_pixels_in_range():
    rs = np.random.RandomState(0)
    seg = rs.randint(-2, 12, size=(3, 17, 9)).astype(np.int32)      # labels -2, -1, 10, 11 are outside [0, 10)
    rmap, off = TG.compact_region_map(seg, 10)
    rmap[1, 4] = -1                                                   # a label without a region
    counts = TG.node_counts(seg, rmap, off, _blobs(rs, 3, 17, 9))
    for i in range(3):
        inside = (seg[i] >= 0) & (seg[i] < 10)
        if i == 1:
            inside &= seg[i] != 4
        assert counts[off[i]:off[i + 1], 0].sum() == inside.sum()
    assert (counts[:, 1:] <= counts[:, :1]).all() and (counts >= 0).all()


def test_reference_band_zero_ignores_no_node_with_pixels():
    rs = np.random.RandomState(1)
    seg = _blocks(2, 20, 20, 5)
    rmap, off = TG.compact_region_map(seg, 20)                        # labels 16 .. 19 do not occur
    mt, it, et, counts = TG.node_targets(seg, rmap, off, _blobs(rs, 2, 20, 20), band_permille=0)
    assert (counts[:, 0] > 0).all() and set(np.unique(mt)) <= {0, 1} and set(np.unique(it)) <= {0, 1} and set(np.unique(et)) <= {0.0, 1.0}
    mt, it, et, _ = TG.targets_from_counts(np.array([[0, 0, 0, 0], [4, 2, 3, 0]]), 0, 1) + (None,)
    assert mt.tolist() == [-1, 0] and it.tolist() == [-1, 1] and et.tolist() == [-1.0, 0.0]       # no pixels; a tie gives 0


def test_reference_boundary_of_a_full_mask_and_of_one_pixel():
    full = np.full((1, 9, 7), 255, np.uint8)
    assert not TG.mask_boundary(full).any()
    one = np.zeros((1, 9, 7), np.uint8)
    one[0, 4, 3] = 200
    b = TG.mask_boundary(one)
    assert b.sum() == 1 and b[0, 4, 3]
    hole = full.copy()
    hole[0, 4, 3] = 127                                               # the four neighbours of a hole, not the hole
    b = TG.mask_boundary(hole)
    assert b.sum() == 4 and b[0, 3, 3] and b[0, 5, 3] and b[0, 4, 2] and b[0, 4, 4]


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(seg, rmap, off, gt, inst=None, edge=None, band=0, emin=1):
    from camouflage_multimodal_amd import node_targets_from_masks
    out = node_targets_from_masks(_dev(seg), _dev(rmap), [int(v) for v in off], _dev(gt), _dev(inst), _dev(edge), band, emin)
    assert [o.dtype for o in out] == [torch.int32, torch.int32, torch.float32, torch.int32] and all(o.is_cuda for o in out)
    return [o.cpu().numpy() for o in out]


def _hold(got, want, tag=""):
    for name, g, w in zip(("mask_t", "inst_t", "edge_t", "counts"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())


def _check(seg, rmap, off, gt, inst=None, edge=None, band=0, emin=1, tag=""):
    want = TG.node_targets(seg, rmap, off, gt, inst, edge, band, emin)
    got = _run(seg, rmap, off, gt, inst, edge, band, emin)
    _hold(got, want, tag)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("given", [False, True])
def test_slic_labels_and_blob_masks_at_a_size_that_is_no_multiple_of_a_tile(given):
    from camouflage_multimodal_amd import create_region_graphs_from_segments, slic_label_bound, slic_segments
    rs = np.random.RandomState(7)
    yy, xx = np.mgrid[0:70, 0:33]
    img = np.stack([np.stack([0.5 + 0.4 * np.sin(yy / (5.0 + i) + c) * np.cos(xx / 4.0) for c in range(3)], -1) for i in range(2)])
    img = torch.from_numpy(np.clip(img + rs.uniform(-0.05, 0.05, img.shape), 0, 1).astype(np.float32)).cuda()
    seg = slic_segments(img, 30)
    graphs, rmap = create_region_graphs_from_segments(img, seg, label_bound=slic_label_bound(70, 33, 30))
    off = graphs.node_offsets
    assert off[2] == graphs.x.shape[0] and off[1] > 3 and off[2] - off[1] > 3
    gt = _blobs(rs, 2, 70, 33)
    inst, edge = (_blobs(rs, 2, 70, 33), _blobs(rs, 2, 70, 33, k=6)) if given else (None, None)
    want = _check(seg.cpu().numpy(), rmap.cpu().numpy(), off, gt, inst, edge, tag=f"slic given={given}")
    assert want[3][:, 0].sum() == 2 * 70 * 33 and want[3][:, 1].sum() == (gt > 127).sum()      # every pixel took part
    assert 0 < want[3][:, 3].sum() and {0, 1} <= set(want[0].tolist())


@pytest.mark.gpu
def test_more_labels_than_slots_and_one_label_for_every_tile():
    rs = np.random.RandomState(3)
    seg = np.arange(1600, dtype=np.int32).reshape(1, 40, 40)          # 1024 labels in the first tile: 960 of them find the table full
    rmap = np.arange(1600, dtype=np.int32).reshape(1, 1600)
    want = _check(seg, rmap, [0, 1600], _blobs(rs, 1, 40, 40), tag="own label")
    assert (want[3][:, 0] == 1).all() and set(want[0].tolist()) == {0, 1} and set(want[2].tolist()) == {0.0, 1.0}
    one = np.zeros((1, 64, 64), np.int32)
    want = _check(one, np.zeros((1, 1), np.int32), [0, 1], _blobs(rs, 1, 64, 64), _blobs(rs, 1, 64, 64), tag="one label")
    assert want[3][0, 0] == 4096


@pytest.mark.gpu
def test_mask_boundary_along_tile_edges_and_the_image_border():
    """The derived boundary needs the neighbour across a tile edge (the halo) and must not see one across the image border."""
    seg = _blocks(4, 70, 70, 7)
    rmap, off = TG.compact_region_map(seg, 100)
    gt = np.zeros((4, 70, 70), np.uint8)
    gt[0, 32:64, 0:32] = 255          # edges on the tile lines y = 32, y = 64, x = 32 and on the image border x = 0
    gt[1, 33:65, 1:33] = 255          # the same mask one pixel off
    gt[2] = 255                       # the whole image: no boundary at all
    gt[3, 0:32, :] = 255              # a band that ends exactly on a tile line and touches three borders
    want = _check(seg, rmap, off, gt, tag="halo")
    per_image = [int(want[3][off[i]:off[i + 1], 3].sum()) for i in range(4)]
    assert per_image == [32 + 32 + 30, 4 * 32 - 4, 0, 70], per_image      # image 0: top, bottom, and the right side between them; no left side


@pytest.mark.gpu
def test_bytes_127_and_128_and_a_tie():
    gt = np.zeros((1, 8, 8), np.uint8)
    gt[0, :, 0::2], gt[0, :, 1::2] = 127, 128
    inst = np.zeros((1, 8, 8), np.uint8)
    inst[0].reshape(-1)[:33] = 128                                     # 33 of 64: a majority by one
    one = np.zeros((1, 8, 8), np.int32)
    want = _check(one, np.zeros((1, 1), np.int32), [0, 1], gt, inst, tag="127 / 128")
    assert want[3].tolist() == [[64, 32, 33, 32]] and want[0].tolist() == [0] and want[1].tolist() == [1]      # 2 pos == pix: 0


BAND_POS = (0, 1, 40, 45, 50, 51, 55, 60, 99, 100)      # positive pixels of ten regions of 100 pixels


@pytest.mark.gpu
@pytest.mark.parametrize("band", [0, 100, 499])
@pytest.mark.parametrize("emin", [1, 3])
def test_band_and_edge_threshold(band, emin):
    seg = _blocks(1, 10, 100, 10)
    rmap, off = TG.compact_region_map(seg, 10)
    gt = np.zeros((1, 10, 100), np.uint8)
    edge = np.zeros((1, 10, 100), np.uint8)
    for k, pos in enumerate(BAND_POS):
        block = np.zeros(100, np.uint8)
        block[:pos] = 255
        gt[0, :, 10 * k:10 * k + 10] = block.reshape(10, 10)
        e = np.zeros(100, np.uint8)
        e[:k % 5] = 255                                                # 0 .. 4 edge pixels
        edge[0, :, 10 * k:10 * k + 10] = e.reshape(10, 10)
    want = _check(seg, rmap, off, gt, None, edge, band, emin, tag=f"band {band} emin {emin}")
    assert want[3][:, 1].tolist() == list(BAND_POS)
    expect = {0: [0, 0, 0, 0, 0, 1, 1, 1, 1, 1], 100: [0, 0, 0, -1, -1, -1, -1, -1, 1, 1], 499: [0, -1, -1, -1, -1, -1, -1, -1, -1, 1]}[band]
    assert want[0].tolist() == expect and want[1].tolist() == expect
    assert want[2].tolist() == [float(k % 5 >= emin) for k in range(10)]
    want = _check(seg, rmap, off, gt, None, None, band, emin, tag=f"band {band} emin {emin}, derived edge")
    assert want[2][0] == 0.0 and want[2][4] == 1.0                            # no positive pixel; five rows of ten above five empty ones


def _excluded_case():
    rs = np.random.RandomState(5)
    seg = _blocks(2, 40, 36, 6).astype(np.int32)                       # 7 x 6 = 42 labels
    seg[0, 0:3, 0:5] = -3
    seg[0, 10, 10:20] = 48                                             # == label_bound
    seg[1, 39, :] = 2 ** 31 - 1
    seg[1, 20:26, 0:6] = 45                                            # in range, but its region_map entry is -1
    mapped = np.where(seg == 45, 44, seg)                              # label 44 gets a region that no pixel carries: the last node of image 1
    mapped[0][seg[0] == 7] = -1                                        # label 7 occurs in image 0 and has no region there
    rmap, off = TG.compact_region_map(mapped, 48)
    assert rmap[0, 7] == -1 and rmap[1, 45] == -1 and rmap[1, 44] == off[2] - off[1] - 1
    return seg, rmap, off, _blobs(rs, 2, 40, 36), _blobs(rs, 2, 40, 36)


@pytest.mark.gpu
def test_excluded_pixels_and_a_node_without_pixels():
    seg, rmap, off, gt, inst = _excluded_case()
    want = _check(seg, rmap, off, gt, inst, tag="excluded")
    n = off[2]
    assert want[3][n - 1].tolist() == [0, 0, 0, 0] and want[0][n - 1] == -1 and want[1][n - 1] == -1 and want[2][n - 1] == -1.0
    taking_part = 2 * 40 * 36 - 15 - 10 - 36 - 36 - int((seg[0] == 7).sum())
    assert want[3][:, 0].sum() == taking_part and (want[3][:n - 1, 0] > 0).all()


@pytest.mark.gpu
def test_rows_past_n_nodes_are_untouched():
    """camo_rg_node_targets called directly with n_nodes below node_off[N]: the pixels of the nodes past it take no part, and the four
    outputs, each of exactly n_nodes rows in the middle of a tensor filled with a sentinel, are written inside their extents only."""
    from raw_calls import BUILDERS, execute
    seg, rmap, off, gt, inst = _excluded_case()
    n = int(off[2]) - 9
    assert off[1] < n < off[2] and rmap.shape[1] == 48
    want = TG.node_targets(seg, rmap, off, gt, inst, None, 100, 2, n_nodes=n)
    assert np.array_equal(want[3], TG.node_counts(seg, rmap, off, gt, inst)[:n])          # the rows below n do not change
    got = execute(BUILDERS["camo_rg_node_targets"](seg, rmap, off, gt, inst, None, n, 100, 2), 0xA5)      # (the reference holds -1 entries)
    got = [got[k] for k in ("mask_t", "inst_t", "edge_t", "counts")]
    _hold(got, want, "n_nodes below node_off[N]")


@pytest.mark.gpu
def test_a_batch_is_its_images_one_by_one_and_two_calls_give_the_same_bytes():
    rs = np.random.RandomState(11)
    seg = np.stack([_blocks(1, 45, 50, b)[0] for b in (5, 9, 25)])      # 90, 30 and 4 nodes
    rmap, off = TG.compact_region_map(seg, 128)
    assert np.diff(off).tolist() == [90, 30, 4]
    gt, inst = _blobs(rs, 3, 45, 50), _blobs(rs, 3, 45, 50)
    whole = _check(seg, rmap, off, gt, inst, None, 100, 2, tag="batch")
    again = _run(seg, rmap, off, gt, inst, None, 100, 2)
    for a, b in zip(whole, again):
        assert a.tobytes() == b.tobytes()
    for i in range(3):
        got = _run(seg[i:i + 1], rmap[i:i + 1], [0, off[i + 1] - off[i]], gt[i:i + 1], inst[i:i + 1], None, 100, 2)
        for a, b in zip(whole, got):
            assert a[off[i]:off[i + 1]].tobytes() == b.tobytes(), i


@pytest.mark.gpu
def test_painted_targets_score_against_the_mask_as_the_counts_predict():
    """paint_regions(mask_t) thresholded and counted by segmentation_counts against the ground truth: TP is the mask-positive pixels
    of the nodes whose target is 1, FP their other pixels, FN every other positive pixel of the image."""
    from camouflage_multimodal_amd import node_targets_from_masks, paint_regions, segmentation_counts
    seg, rmap, off, gt, _ = _excluded_case()
    d_seg, d_rmap, d_gt = _dev(seg), _dev(rmap), _dev(gt)
    offs = [int(v) for v in off]
    mt, it, et, counts = node_targets_from_masks(d_seg, d_rmap, offs, d_gt)
    painted = paint_regions(mt.to(torch.float32), d_seg, d_rmap, offs, fill=0.0)
    got = segmentation_counts(painted[:, 0], d_gt, 0.5).cpu().numpy()
    c, t = TG.node_counts(seg, rmap, off, gt), TG.node_targets(seg, rmap, off, gt)[0]
    assert np.array_equal(counts.cpu().numpy(), c.astype(np.int32)) and np.array_equal(mt.cpu().numpy(), t)
    for i in range(2):
        sl = slice(off[i], off[i + 1])
        on = t[sl] == 1
        tp, fp = int(c[sl][on, 1].sum()), int((c[sl][on, 0] - c[sl][on, 1]).sum())
        fn = int((gt[i] > 127).sum()) - tp
        assert got[i, :4].tolist() == [tp, fp, fn, 40 * 36 - tp - fp - fn], i
        assert tp > 0 and fp > 0 and fn > 0
