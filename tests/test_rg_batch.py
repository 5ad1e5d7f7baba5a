"""Batched region-graph construction (include/camo_rg_batch.h) and the batched image -> prediction surface on top of it.

PARITY UNPINNED as for test_rg_features.py: the checker is oracle/rg_features_oracle.py, applied image by image to the fp32
images the device gets.  Bounds against the oracle are test_region_graph_kernels_match_oracle's own (x within 2e-6 column
scale + 2e-6 |x|, edge weights within 2e-5 w + 1e-9) on inputs that carry 0.05 noise, so that no region is flat; on flat regions
the header's derived bound is held instead (std <= sqrt(CAMO_RGB_VAR_BOUND), means exactly the colour).  The sums are integers,
so "twice the same call" and "a batch against its images one by one" are held byte for byte, flat regions included.

Images to predictions (test 7): predict_batch_from_images in f32 against predict_from_image image by image regroups twice --
packed batch against B x (B = 1) (2e-6 on probabilities and score, 4e-6 on logits: test_predict_batch.py) and the GNN on the
block-diagonal batch against separate graphs (1e-5 max(|emb|, 1): test_rg_gnn.py) -- and the bound is the sum of the two.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import slic_ref as R
from conftest import ROOT
from oracle import rg_features_oracle as RO
from rg_maps import FLAT_A, FLAT_B, check_against_oracle as _check_against_oracle, flat


def _flat():
    """rg_maps.flat(0): a saturated two-colour image whose regions are flat (every region of a 12-region map has one of two colours)."""
    return flat(0)


def _inputs(H, W, n, seed):
    """test_rg_features.py's inputs, the image as the fp32 array the device gets."""
    rs = np.random.RandomState(seed)
    seg = RO.voronoi_segments(H, W, n, seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    img = np.clip(np.stack([0.5 + 0.4 * np.sin(7 * xx + seed), 0.5 + 0.4 * np.cos(5 * yy), xx * yy], -1) + 0.05 * rs.standard_normal((H, W, 3)), 0, 1)
    canny = rs.uniform(0, 1, (H, W)) > 0.85
    return img.astype(np.float32), seg, canny


def _stack(cases):
    parts = [_inputs(*c) for c in cases]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


@functools.lru_cache(maxsize=None)
def _mixed():
    """Test 1's batch: 7, 23, 1 and 40 regions at 64 x 48; the 40-region map has label 17 merged away.  Never written to."""
    img, seg, canny = _stack([(64, 48, 7, 2), (64, 48, 23, 3), (64, 48, 1, 4), (64, 48, 40, 5)])
    seg[3][seg[3] == 17] = 18
    return img, seg, canny


@functools.lru_cache(maxsize=None)
def _oracle(key):
    img, seg, canny = {"mixed": _mixed}[key]()
    return [RO.region_graph(img[k], seg[k], canny[k]) for k in range(len(img))]


def _build(img, seg, canny, **kw):
    from camouflage_multimodal_amd import create_region_graphs_from_segments
    return create_region_graphs_from_segments(torch.from_numpy(np.ascontiguousarray(img)).cuda(), torch.from_numpy(np.ascontiguousarray(seg)).cuda(),
                                              None if canny is None else torch.from_numpy(np.ascontiguousarray(canny)).cuda(), **kw)


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_binding_and_refusals_without_a_gpu():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_rg_batch.h")).read()
    assert "PARITY UNPINNED" in hdr
    assert _lib.ABI_VERSION == 13 and _lib.lib().camo_abi_version() == 13
    assert int(re.search(r"#define CAMO_RGB_TILE_SLOTS (\d+)", hdr).group(1)) == _lib.RGB_TILE_SLOTS
    S = int(re.search(r"#define CAMO_RGB_FIX_BITS (\d+)", hdr).group(1))
    assert float(re.search(r"#define CAMO_RGB_VAR_BOUND ([0-9.e+-]+)", hdr).group(1)) == 3 * 2.0 ** -(S + 1) == _lib.RGB_VAR_BOUND
    L = _lib.lib()
    need = L.camo_rg_batch_workspace_bytes(2, 64, 48, 41)
    assert need >= 2 * 41 * (21 * 8 + 2 * 4 + 8)
    sizes = [L.camo_rg_batch_workspace_bytes(n, 256, 256, 600) for n in (1, 2, 3, 16, 17)]
    assert all(a > 0 for a in sizes) and all(a < b for a, b in zip(sizes, sizes[1:]))      # monotone in N

    def call(N=2, H=64, W=48, lb=41, nbytes=need, nodes=None, cap=64):
        return L.camo_rg_region_graph_batch(None, None, None, N, H, W, lb, None, nbytes, None, N * lb if nodes is None else nodes, None, None, None,
                                            cap, None, None, None, None, None)
    for kw, code, text in ((dict(N=0), -1, b"N >= 1"), (dict(lb=0), -1, b"label_bound"), (dict(lb=4097), -1, b"label_bound"),
                           (dict(nbytes=need - 1), -3, b"camo_rg_batch_workspace_bytes"), (dict(H=8193, W=8193, N=1), -2, b"IMAGE_PIXELS"),
                           (dict(N=4097), -2, b"MAX_IMAGES"), (dict(N=64, H=2048, W=2048), -2, b"MAX_PIXELS"), (dict(nodes=81), -1, b"node_capacity"),
                           (dict(cap=1), -1, b"edge_capacity"), (dict(), -1, b"null")):
        assert call(**kw) == code and text in L.camo_last_error(), (kw, L.camo_last_error())
    assert L.camo_rg_batch_workspace_bytes(0, 64, 48, 41) == 0 and b"N >= 1" in L.camo_last_error()
    assert L.camo_rg_batch_workspace_bytes(1, 8193, 8193, 41) == 0 and b"IMAGE_PIXELS" in L.camo_last_error()
    assert L.camo_rg_batch_workspace_bytes(1, 64, 48, 4097) == 0


def test_wrappers_need_a_device_and_matching_shapes():
    import camouflage_multimodal_amd as pkg
    from camouflage_multimodal_amd import (RegionGraphBatch, _lib, create_region_graphs_from_segments, predict_batch_from_images,
                                           region_graphs_from_images)
    for name in ("RegionGraphBatch", "create_region_graphs_from_segments", "region_graphs_from_images", "predict_batch_from_images"):
        assert name in pkg.__all__
    img, seg, canny = _stack([(16, 16, 4, 0), (16, 16, 3, 1)])
    with pytest.raises(_lib.CamoError):
        create_region_graphs_from_segments(img, seg, canny, device="cpu")
    with pytest.raises(_lib.CamoError):
        region_graphs_from_images(torch.zeros(2, 16, 16, 3), 4)
    with pytest.raises(_lib.CamoError):
        predict_batch_from_images(None, None, img, {}, "cpu", n_segments=4)
    for bad in ((img[0], seg, canny), (img, seg[0], canny), (img, seg, canny[0]), (img, seg[:, :8], canny), (img[..., :2], seg, canny)):
        with pytest.raises(ValueError, match="need images"):
            create_region_graphs_from_segments(*bad, device="cpu")
    with pytest.raises(ValueError, match="need images"):
        region_graphs_from_images(img[0], 4, device="cpu")
    g = RegionGraphBatch(torch.zeros(5, 15), torch.tensor([[0, 1, 3, 4], [1, 0, 4, 3]]), torch.ones(4, 1), torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32),
                         [0, 2, 5], [0, 2, 4])
    parts = g.to("cpu").graphs()
    assert g.num_graphs == 2 and [tuple(p.x.shape) for p in parts] == [(2, 15), (3, 15)]
    assert parts[1].edge_index.tolist() == [[1, 2], [2, 1]] and parts[1].edge_attr.shape == (2, 1)


def test_label_bound_holds_on_the_reference_connect_step():
    from camouflage_multimodal_amd import slic_label_bound
    cases = R.cases()
    for name in R.CLEAR:
        H, W, n, (_, _, _, _, K) = R.TABLE[name]
        bound = slic_label_bound(H, W, n)
        assert bound == H * W // max(int(0.5 * H * W / K), 1) + 2
        for image in cases[name][0]:
            labels = R.slic(image, n)[0]
            assert 0 <= labels.min() and labels.max() < bound, (name, int(labels.max()), bound)
    assert slic_label_bound(256, 256, 500) == 256 * 256 // 61 + 2
    assert slic_label_bound(2048, 2048, 3900) <= 4096


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_mixed_batch_matches_oracle():
    img, seg, canny = _mixed()
    want = _oracle("mixed")
    assert want[2][1].shape[1] == 0 and want[3][3][17] == -1            # an image without edges; an empty label besides 0
    g, rm = _build(img, seg, canny)
    assert rm.shape == (4, 41) and g.edge_offsets[2] == g.edge_offsets[3]
    _check_against_oracle(g, rm, want, "mixed batch")


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,n", [(2, 33, 70, 60), (1, 256, 256, 500)])
def test_tile_edges_match_oracle(N, H, W, n):
    img, seg, canny = _stack([(H, W, n, 3 + k) for k in range(N)])
    for k in range(N):
        seg[k][seg[k] == 5] = 6
    # regions on every tile border: some row / column next to each border holds two labels across it
    for b in range(32, H, 32):
        assert (seg[0][b - 1] != seg[0][b]).any()
    for b in range(32, W, 32):
        assert (seg[0][:, b - 1] != seg[0][:, b]).any()
    want = [RO.region_graph(img[k], seg[k], canny[k]) for k in range(N)]
    g, rm = _build(img, seg, canny)
    _check_against_oracle(g, rm, want, f"{N} x {H} x {W}")


@pytest.mark.gpu
def test_hash_table_overflow_matches_oracle():
    from camouflage_multimodal_amd import _lib
    img, seg, canny = _stack([(64, 64, 600, 6)])
    per_tile = [len(np.unique(seg[0][y:y + 32, x:x + 32])) for y in (0, 32) for x in (0, 32)]
    assert max(per_tile) > _lib.RGB_TILE_SLOTS, per_tile               # asserted before the device is asked
    want = [RO.region_graph(img[0], seg[0], canny[0])]
    g, rm = _build(img, seg, canny)
    _check_against_oracle(g, rm, want, f"overflow ({max(per_tile)} labels in a tile)")


def _bytes(g, rm):
    return [t.cpu().numpy().tobytes() for t in (g.x, g.edge_index, g.edge_attr, g.batch, rm)] + [tuple(g.node_offsets), tuple(g.edge_offsets)]


@pytest.mark.gpu
def test_two_calls_and_batch_against_singles_byte_for_byte():
    from camouflage_multimodal_amd import _lib
    mi, ms, mc = _mixed()
    fi, fs, fc = _flat()
    img, seg, canny = np.concatenate([mi, fi[None]]), np.concatenate([ms, fs[None]]), np.concatenate([mc, fc[None]])
    g, rm = _build(img, seg, canny, label_bound=41)
    g2, rm2 = _build(img, seg, canny, label_bound=41)
    assert _bytes(g, rm) == _bytes(g2, rm2)
    no, eo = g.node_offsets, g.edge_offsets
    for k in range(5):
        g1, rm1 = _build(img[k:k + 1], seg[k:k + 1], canny[k:k + 1], label_bound=41)
        assert g1.node_offsets == [0, no[k + 1] - no[k]] and g1.edge_offsets == [0, eo[k + 1] - eo[k]], k
        assert g1.x.cpu().numpy().tobytes() == g.x[no[k]:no[k + 1]].cpu().numpy().tobytes(), k
        assert g1.edge_attr.cpu().numpy().tobytes() == g.edge_attr[eo[k]:eo[k + 1]].cpu().numpy().tobytes(), k
        assert (g1.edge_index.cpu() == g.edge_index[:, eo[k]:eo[k + 1]].cpu() - no[k]).all(), k
        assert (rm1.cpu() == rm[k:k + 1].cpu()).all() and (g1.batch.cpu() == 0).all() and (g.batch[no[k]:no[k + 1]].cpu() == k).all(), k
    # the flat regions: means exactly the colour, std within the square root of the header's variance bound
    x = g.x[no[4]:no[5]].cpu().numpy()
    labels = np.unique(fs)
    assert len(labels) == x.shape[0] == 12
    for row, lab in zip(x, labels):
        assert row[:3].tobytes() == (FLAT_A if lab % 2 == 0 else FLAT_B).tobytes(), (lab, row[:3])
    std = np.abs(x[:, [3, 4, 5, 7]]).max()
    print(f"flat regions: largest std feature {std:.3e}, bound {np.sqrt(_lib.RGB_VAR_BOUND):.3e}; largest luma variance {x[:, 14].max():.3e}")
    assert std <= np.sqrt(_lib.RGB_VAR_BOUND) and x[:, 14].max() <= _lib.RGB_VAR_BOUND


@pytest.mark.gpu
def test_small_capacity_is_regrown_and_labels_out_of_range_raise():
    img, seg, canny = _mixed()
    want = _oracle("mixed")
    g, rm = _build(img, seg, canny, edge_capacity=64)                   # far too small: reported, regrown
    assert g.edge_index.shape[1] == sum(w[1].shape[1] for w in want) > 64
    _check_against_oracle(g, rm, want, "regrown")
    bad = seg.copy()
    bad[1, 10, 10] = 41
    with pytest.raises(ValueError, match=r"\b1 pixel\b"):
        _build(img, bad, canny, label_bound=41)
    bad = seg.copy()
    bad[2, 0, 0] = -3
    with pytest.raises(ValueError, match=r"\b1 pixel\b"):
        _build(img, bad, canny)
    bad[0, 63, 47] = 4000
    with pytest.raises(ValueError, match=r"\b2 pixels\b"):
        _build(img, bad, canny, label_bound=41)


def _gnn():
    from camouflage_multimodal_amd import RegionGraphGNN
    torch.manual_seed(0)
    m = RegionGraphGNN().cuda().eval()
    for bn in (m.bn1, m.bn2, m.bn3, m.bn4):
        bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    return m


@pytest.mark.gpu
def test_batch_feeds_the_gnn_like_its_graphs_one_by_one():
    img, seg, canny = _mixed()
    g, _ = _build(img, seg, canny)
    m = _gnn()
    emb = m.extract_node_embeddings(g)
    parts = [m.extract_node_embeddings(d) for d in g.graphs()]
    # test_hip_batched_graphs_equal_separate_graphs_and_unweighted_edges' bound for a batch against separate graphs
    tol = 1e-5 * max(float(emb.abs().max()), 1.0)
    d = float((emb - torch.cat(parts)).abs().max())
    print(f"GNN on the batch vs per image: {d:.3e} (bound {tol:.3e})")
    assert emb.shape == (g.node_offsets[-1], 128) and d < tol
    pooled = m.extract_graph_embedding(g)
    assert pooled.shape == (4, 128)
    assert float((pooled - torch.stack([p.mean(0) for p in parts])).abs().max()) < tol


def _images_96x80():
    return np.concatenate([R.cases()["96x80"][0], R.noise_image(96, 80, 11)[None]])


@pytest.mark.gpu
def test_graphs_from_images_match_oracle_on_the_device_segments():
    """region_graphs_from_images on the 96 x 80 SLIC case (blob image, noise image) plus a noise image of this file's: segments
    byte-equal to slic_segments, graphs at test 1's bounds against the oracle on those segments and the device Canny map.

    Image 0 (the blob image) saturates to regions of one flat colour, where the oracle's std is 0: the squares are summed exactly
    (include/camo_rg_batch.h), so the device gives 0 there as well.  The figures are printed before the assertion."""
    from camouflage_multimodal_amd import canny_edges, region_graphs_from_images, slic_segments
    images = _images_96x80()
    dev = torch.from_numpy(images).cuda()
    g, seg = region_graphs_from_images(dev, 60)
    assert seg.dtype == torch.int32 and seg.cpu().numpy().tobytes() == slic_segments(dev, 60).cpu().numpy().tobytes()
    segs, canny = seg.cpu().numpy(), canny_edges(dev).cpu().numpy()
    want = [RO.region_graph(images[k], segs[k], canny[k]) for k in range(3)]
    rm = torch.full((3, max(len(w[3]) for w in want)), -1, dtype=torch.int32)
    for k, w in enumerate(want):                                         # (region_graphs_from_images does not return the map: the oracle's stands in, the rest is checked)
        rm[k, :len(w[3])] = torch.from_numpy(w[3])
    gx = g.x.cpu().numpy()
    for k, w in enumerate(want):
        xs = gx[g.node_offsets[k]:g.node_offsets[k + 1]]
        if xs.shape == w[0].shape:
            bound = 2e-6 * np.maximum(np.abs(w[0]).max(0), 1e-3) + 2e-6 * np.abs(w[0])
            print(f"image {k}: worst |x - oracle| / bound per column {np.round((np.abs(xs - w[0]) / bound).max(0), 3).tolist()}")
    _check_against_oracle(g, rm, want, "96 x 80 from the images")


@pytest.mark.gpu
def test_images_to_predictions_in_one_batch(kg_real):
    from camouflage_multimodal_amd import (RegionGraphGNN, build_multimodal_model, predict_batch_from_images, predict_from_image,
                                           region_graph_from_image, region_graphs_from_images)
    images = _images_96x80()
    dev = torch.from_numpy(images).cuda()
    g, _ = region_graphs_from_images(dev, 60)
    no = g.node_offsets
    torch.manual_seed(1)
    rgm = RegionGraphGNN().cuda().eval()
    fm = build_multimodal_model({}).cuda().eval().set_precision("f32")
    kg = {f"cat{i:02d}": torch.from_numpy(kg_real[i:i + 1]) for i in range(13)}
    preds, attn, _ = predict_batch_from_images(fm, rgm, dev, kg, "cuda", n_segments=60)
    assert len(preds) == len(attn) == 3
    emb = rgm.extract_node_embeddings(g)
    gnn_tol = 1e-5 * max(float(emb.abs().max()), 1.0)                    # batch against separate graphs (test_rg_gnn.py)
    worst = [0.0, 0.0, 0.0, 0.0]
    fails = []
    for k in range(3):
        one, _, _ = predict_from_image(fm, rgm, dev[k], kg, "cuda", n_segments=60)
        # measured, not asserted: the two constructions' x through the same GNN on the same edges
        d1, _ = region_graph_from_image(dev[k], 60)
        gk = g.graphs()[k]
        assert d1.x.shape == gk.x.shape and (d1.edge_index == gk.edge_index).all()
        dx = float((d1.x - gk.x).abs().max())
        de = float((rgm.extract_node_embeddings(x=d1.x, edge_index=gk.edge_index, edge_attr=d1.edge_attr) -
                    rgm.extract_node_embeddings(x=gk.x, edge_index=gk.edge_index, edge_attr=gk.edge_attr)).abs().max())
        p = preds[k]
        dl = max(float((p[key] - one[key]).abs().max()) for key in ("mask_logits",))
        dp = max(float((p[key] - one[key]).abs().max()) for key in ("mask_prob", "instance_prob"))
        dp = max(dp, abs(p["edge_prob"] - one["edge_prob"]), abs(p["score"] - one["score"]))
        worst = [max(a, b) for a, b in zip(worst, (dx, de, dl, dp))]
        print(f"image {k}: |x f64-atomic - x integer| {dx:.3e}, through the GNN {de:.3e}; batch vs per image: logits {dl:.3e}, probabilities / score {dp:.3e}")
        assert p["mask_pred"] == one["mask_pred"] and p["instance_pred"] == one["instance_pred"]
        nr = no[k + 1] - no[k]
        assert attn[k]["rg2kg"].shape == (nr, 13) and attn[k]["kg2rg"].shape == (13, nr)
        if not (dl <= 4e-6 + gnn_tol and dp <= 2e-6 + gnn_tol):
            fails.append((k, dl, dp))
    print(f"images to predictions: bounds logits {4e-6 + gnn_tol:.3e}, probabilities / score {2e-6 + gnn_tol:.3e}; worst x {worst[0]:.3e}, "
          f"GNN {worst[1]:.3e}, logits {worst[2]:.3e}, probabilities / score {worst[3]:.3e}")
    assert not fails, fails
