"""The region-graph detector (include/camo_rg_detect.h) against tests/rg_detect_ref.py.

PARITY UNPINNED (the reference tree, torch_geometric, scikit-image and an RG checkpoint are absent): the header is the definition
and the numpy restatement the checker.  CPU tests hold the restatement to brute force and to hand cases and the library's
argument checks to the header; GPU tests hold the kernels to the restatement:

  heads     logits within 2e-5 max|ref| + 2e-6 of float64 (the bound the GNN that feeds them is held to), probabilities within
            half of that + 2e-6 (softmax over a logit difference and the sigmoid have slope <= 1/4; the fast exponential adds a few ulp)
  paint     bit for bit (a gather)
  counts    all five integers equal, two calls the same bytes, a batch the rows of its images
  end to end  nothing compared across a threshold between two arithmetic paths: the maps against the call's own node
            probabilities, the metrics against the counts of the call's own maps
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import rg_detect_ref as R
from conftest import ROOT
from oracle import rg_features_oracle as FO
from oracle import rg_gnn_oracle as RO

_rows = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "rg_detect.h")).read()
T = int(re.search(r"RGD_ROWS = (\d+)", _rows).group(1))                # the heads kernel's row tile at hidden <= RGD_WIDE_ABOVE
TW = int(re.search(r"RGD_ROWS_WIDE = (\d+)", _rows).group(1))          # ... above it
WIDE_ABOVE = int(re.search(r"RGD_WIDE_ABOVE = (\d+)", _rows).group(1))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _paint_batch():
    """N = 3 at 33 x 70 (no multiple of any tile): Voronoi maps of 7, 1 and 40 regions; the third has an empty label in the middle
    (21), so region_map is -1 there; label_bound 45 lies above the largest label (41); the first image holds one pixel with the
    label 45 = label_bound and one with a negative label.  Returns (segments, region_map, node_off); never written to."""
    segs = np.stack([FO.voronoi_segments(33, 70, n, 30 + i) for i, n in enumerate((7, 1, 40))]).astype(np.int32)
    segs[2][segs[2] > 20] += 1
    segs[0, 0, 0] = 45
    segs[0, 5, 5] = -3
    rmap, off = R.region_map_of(segs, 45)
    assert rmap[2, 21] == -1 and rmap[2, 20] >= 0 and rmap[2, 22] >= 0 and list(off) == [0, 7, 8, 48] and (rmap[:, 0] == -1).all()
    for a in (segs, rmap, off):
        a.setflags(write=False)
    return segs, rmap, off


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_header_symbols_binding_and_abi_version():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_rg_detect.h")).read()
    assert "PARITY UNPINNED" in hdr and "utils/metrics.py" in hdr
    assert _lib.ABI_VERSION == 13 and "#define CAMO_ABI_VERSION 13" in open(os.path.join(ROOT, "include", "camo_fusion.h")).read()
    assert _lib.lib().camo_abi_version() == 13
    assert int(re.search(r"CAMO_RGD_MAX_CHANNELS (\d+)", hdr).group(1)) == _lib.RGD_MAX_CHANNELS
    assert int(re.search(r"CAMO_RGD_FIX_BITS (\d+)", hdr).group(1)) == _lib.RGD_FIX_BITS == 32
    names = re.findall(r"\b(CAMO_RGD_(?:MASK|INST|EDGE)_[WB][12])\b", hdr.split("enum {")[1].split("}")[0])
    assert len(names) == _lib.RGD_NPARAMS == len(R.head_specs())


def test_reference_counts_against_a_python_loop_on_5x7():
    rs = np.random.RandomState(0)
    pred = rs.uniform(0, 1, (2, 5, 7)).astype(np.float32)
    pred[0, 0, :3] = (0.5, 0.0, 1.0)
    gt = rs.choice(np.array([0, 127, 128, 255], np.uint8), (2, 5, 7))
    want = np.zeros((2, 5), np.int64)
    for i in range(2):
        for y in range(5):
            for x in range(7):
                v, g = float(pred[i, y, x]), 1 if int(gt[i, y, x]) > 127 else 0
                p = 1 if v > 0.5 else 0
                want[i, {(1, 1): 0, (1, 0): 1, (0, 1): 2, (0, 0): 3}[(p, g)]] += 1
                want[i, 4] += int(round(abs(v - g) * 2 ** 32))             # (round and rint both take a half to even)
    got = R.counts(pred, gt, 0.5)
    assert got.dtype == np.int64 and np.array_equal(got, want) and (got[:, :4].sum(1) == 35).all()


def test_ratio_conventions_on_hand_cases():
    from camouflage_multimodal_amd import segmentation_metrics
    cases = {"both empty": ([0, 0, 0, 35, 0], dict(iou=1.0, dice=1.0, precision=0.0, recall=0.0, f1=0.0, accuracy=1.0, mae=0.0)),
             "prediction empty": ([0, 0, 10, 25, 10 * 2 ** 32], dict(iou=0.0, dice=0.0, precision=0.0, recall=0.0, f1=0.0, accuracy=25 / 35, mae=10 / 35)),
             "ground truth empty": ([0, 7, 0, 28, 7 * 2 ** 32], dict(iou=0.0, dice=0.0, precision=0.0, recall=0.0, f1=0.0, accuracy=28 / 35, mae=0.2)),
             "perfect": ([12, 0, 0, 23, 0], dict(iou=1.0, dice=1.0, precision=1.0, recall=1.0, f1=1.0, accuracy=1.0, mae=0.0)),
             "mixed": ([3, 1, 2, 29, 2 ** 31], dict(iou=0.5, dice=6 / 9, precision=0.75, recall=0.6, f1=2 * 0.75 * 0.6 / 1.35, accuracy=32 / 35, mae=0.5 / 35))}
    for name, (row, want) in cases.items():
        ref = R.ratios(row, 5, 7)
        pkg = segmentation_metrics([row], 5, 7)[0]
        for k, v in want.items():
            assert abs(ref[k] - v) < 1e-15 and ref[k] == pkg[k], (name, k, ref[k], pkg[k], v)
        assert [pkg[k] for k in ("tp", "fp", "fn", "tn")] == row[:4]


def test_reference_paint_with_an_identity_region_map():
    rs = np.random.RandomState(1)
    seg = rs.randint(0, 6, (1, 4, 9)).astype(np.int32)
    val = rs.standard_normal((6, 3)).astype(np.float32)
    out = R.paint(val, seg, np.arange(6, dtype=np.int32)[None], np.array([0, 6], np.int32))
    assert out.shape == (1, 3, 4, 9) and np.array_equal(_bits(out[0]), _bits(val[seg[0]].transpose(2, 0, 1)))
    segs, rmap, off = _paint_batch()
    out = R.paint(np.arange(48, dtype=np.float32)[:, None] + 1, segs, rmap, off, fill=-1.0)
    assert out[0, 0, 0, 0] == -1 and out[0, 0, 5, 5] == -1 and (out[1] == 8).all() and (out[2] >= 9).all() and int((out[0] == -1).sum()) == 2
    assert set(np.unique(out[2])) == set(np.arange(9, 49, dtype=np.float32))


def test_reference_heads_shapes_and_probabilities():
    p = R.make_head_params(0, 128, 3)
    l = R.heads(p, np.abs(np.random.RandomState(0).standard_normal((5, 128))).astype(np.float32))
    pr = R.probabilities(l, 3)
    assert l.shape == (5, 7) and pr.shape == (5, 3) and (pr > 0).all() and (pr < 1).all()
    two = R.probabilities(np.array([[0.3, 1.1, -2.0, 0.5, 0.7]]), 2)           # two classes: softmax[1] = sigmoid(l1 - l0)
    assert np.allclose(two[0], [1 / (1 + np.exp(-0.8)), 1 / (1 + np.exp(-2.5)), 1 / (1 + np.exp(-0.7))], rtol=0, atol=1e-15)


def test_training_mode_forward_and_cpu_inputs_raise():
    from camouflage_multimodal_amd import (RegionGraphGNN, attention_to_pixels, detect_camouflage, detect_camouflage_batch, paint_regions,
                                           segmentation_counts)
    from camouflage_multimodal_amd._lib import CamoError
    m = RegionGraphGNN()
    assert m.training and m.num_classes == 2
    with pytest.raises(CamoError, match="training"):
        m(None)
    x, ei, ew = RO.make_graph(9, seed=1)
    data = type("Data", (), dict(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei), edge_attr=torch.from_numpy(ew).unsqueeze(1)))()
    with pytest.raises(CamoError, match="training"):
        m(data)
    m.eval()
    with pytest.raises(CamoError, match="no CPU"):                           # eval mode, CPU tensors: no fallback
        m(data)
    with pytest.raises(CamoError):
        m.node_probabilities(data)
    with pytest.raises(CamoError):
        m.node_heads(torch.zeros(4, 128))
    seg, rmap = torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(CamoError):
        paint_regions(torch.zeros(1, 3), seg, rmap, [0, 1])
    with pytest.raises(CamoError):
        attention_to_pixels([torch.zeros(13, 1)], seg, rmap, [0, 1])
    with pytest.raises(CamoError):
        segmentation_counts(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(CamoError):
        detect_camouflage_batch(m, torch.zeros(2, 16, 16, 3))
    with pytest.raises(CamoError):
        detect_camouflage(m, torch.zeros(16, 16, 3))


def test_argument_checks_without_a_gpu():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)                                              # (never dereferenced: every check comes before any launch)
    table = (ctypes.c_void_p * 12)(*([0x1000] * 12))
    holed = (ctypes.c_void_p * 12)(*([0x1000] * 5 + [0] + [0x1000] * 6))

    def heads(hidden=128, nc=2, tab=table, emb=p, n=4, logits=p, probs=p, dims=True):
        d = _lib.CamoRgDims(15, hidden, 4)
        return L.camo_rg_node_heads(ctypes.byref(d) if dims else None, nc, tab, emb, n, logits, probs, None)
    assert heads(dims=False) == -1 and b"dims" in L.camo_last_error()
    assert heads(hidden=514) == -1 and b"hidden" in L.camo_last_error()
    assert heads(hidden=127) == -1 and heads(hidden=0) == -1
    assert heads(nc=1) == -1 and b"num_classes" in L.camo_last_error()
    assert heads(nc=9) == -1
    assert heads(n=0) == -1 and b"n >= 1" in L.camo_last_error()
    assert heads(tab=None) == -1 and heads(emb=None) == -1 and heads(logits=None) == -1 and heads(probs=None) == -1
    assert b"null" in L.camo_last_error()
    assert heads(tab=holed) == -1 and b"parameter table" in L.camo_last_error()

    def paint(values=p, n=5, C=3, seg=p, rmap=p, off=p, N=1, H=8, W=8, lb=4, maps=p):
        return L.camo_rg_paint(values, n, C, seg, rmap, off, N, H, W, lb, 0.0, maps, None)
    assert paint(C=0) == -1 and paint(C=17) == -1 and b"CAMO_RGD_MAX_CHANNELS" in L.camo_last_error()
    assert paint(n=0) == -1 and paint(N=0) == -1 and paint(H=0) == -1 and paint(W=-1) == -1 and paint(lb=0) == -1
    assert paint(N=64, H=8192, W=8192) == -1 and b"MAX_PIXELS" in L.camo_last_error()
    for k in ("values", "seg", "rmap", "off", "maps"):
        assert paint(**{k: None}) == -1 and b"null" in L.camo_last_error(), k

    def counts(pred=p, stride=64, gt=p, thr=0.5, N=1, H=8, W=8, out=p):
        return L.camo_seg_counts(pred, stride, gt, thr, N, H, W, out, None)
    assert counts(N=0) == -1 and counts(H=0) == -1 and counts(W=0) == -1
    assert counts(N=65536) == -1 and b"MAX_IMAGES" in L.camo_last_error()
    assert counts(H=8193, W=8192, stride=1 << 40) == -1 and b"MAX_IMAGE_PIXELS" in L.camo_last_error()
    assert counts(stride=63) == -1 and b"stride" in L.camo_last_error()
    assert counts(thr=float("nan")) == -1 and b"NaN" in L.camo_last_error()
    assert counts(pred=None) == -1 and counts(gt=None) == -1 and counts(out=None) == -1 and b"null" in L.camo_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _model(hidden, nc, params):
    from camouflage_multimodal_amd import RegionGraphGNN
    m = RegionGraphGNN(hidden_channels=hidden, num_classes=nc)
    sd = m.state_dict()
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


HEAD_CASES = [(128, nc, n) for nc in (2, 3) for n in (1, T - 1, T, T + 1, 530, 2000)] + [(64, 2, T + 1)] \
    + [(WIDE_ABOVE + 128, nc, n) for nc, n in ((2, TW - 1), (2, TW), (3, TW + 1), (8, 41))]        # (the other row tile, and the most classes)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,nc,n", HEAD_CASES)
def test_heads_match_float64(hidden, nc, n):
    assert T == 16 and TW == 8 and WIDE_ABOVE == 256
    p = R.make_head_params(hidden + nc, hidden, nc)
    emb = np.maximum(np.random.RandomState(n).standard_normal((n, hidden)), 0).astype(np.float32)     # like post-ReLU embeddings
    logits, probs = _model(hidden, nc, p).node_heads(torch.from_numpy(emb).cuda())
    logits, probs = logits.cpu().numpy(), probs.cpu().numpy()
    want = R.heads(p, emb)
    wantp = R.probabilities(want, nc)
    bound = 2e-5 * float(np.abs(want).max()) + 2e-6
    el, ep = float(np.abs(logits - want).max()), float(np.abs(probs - wantp).max())
    print(f"hidden {hidden} classes {nc} n {n}: max |logits - float64| = {el:.3e} (bound {bound:.3e}), "
          f"max |probs - float64| = {ep:.3e} (bound {bound / 2 + 2e-6:.3e}), max |ref| = {float(np.abs(want).max()):.3f}")
    assert logits.shape == (n, 2 * nc + 1) and probs.shape == (n, 3) and np.isfinite(logits).all() and np.isfinite(probs).all()
    assert el <= bound
    assert ep <= bound / 2 + 2e-6


@pytest.mark.gpu
def test_forward_is_the_heads_on_the_node_embeddings():
    """Byte for byte on the embeddings forward itself obtained from extract_node_embeddings (recorded by wrapping the method: a
    second extract_node_embeddings call may differ in its last bits, since the CSR builder allocates a row's edge slots with
    atomics); a block-diagonal batch of three graphs against its graphs one by one at the GNN's batch bound."""
    params = dict(RO.make_params(5), **R.make_head_params(6))
    m = _model(128, 2, params)
    x, ei, ew = RO.make_graph(65, seed=14)
    data = type("Data", (), dict(x=torch.from_numpy(x).cuda(), edge_index=torch.from_numpy(ei).cuda(), edge_attr=torch.from_numpy(ew).cuda().unsqueeze(1)))()
    seen = []
    inner = m.extract_node_embeddings
    m.extract_node_embeddings = lambda *a, **k: (seen.append(inner(*a, **k)), seen[-1])[1]
    mask, inst, edge = m(data)
    del m.extract_node_embeddings
    assert len(seen) == 1 and mask.shape == (65, 2) and inst.shape == (65, 2) and edge.shape == (65, 1)
    assert mask._base is not None and mask._base is inst._base and inst._base is edge._base        # views of the one logits tensor
    logits, probs = m.node_heads(seen[0])
    assert torch.equal(torch.cat([mask, inst, edge], dim=1), logits)
    assert torch.equal(m.node_heads(seen[0])[1], probs)
    again = m.extract_node_embeddings(data)
    assert float((again - seen[0]).abs().max()) <= 1e-5 * max(float(again.abs().max()), 1.0)

    gs = [RO.make_graph(n, seed=20 + i) for i, n in enumerate((40, 77, 5))]
    off = np.cumsum([0] + [g[0].shape[0] for g in gs])
    one = [torch.cat(m(type("Data", (), dict(x=torch.from_numpy(g[0]).cuda(), edge_index=torch.from_numpy(g[1]).cuda(),
                                             edge_attr=torch.from_numpy(g[2]).cuda().unsqueeze(1)))()), dim=1) for g in gs]
    batch = type("Data", (), dict(x=torch.from_numpy(np.concatenate([g[0] for g in gs])).cuda(),
                                  edge_index=torch.from_numpy(np.concatenate([g[1] + off[i] for i, g in enumerate(gs)], axis=1)).cuda(),
                                  edge_attr=torch.from_numpy(np.concatenate([g[2] for g in gs])).cuda().unsqueeze(1)))()
    ob = torch.cat(m(batch), dim=1)
    assert ob.shape == (122, 5) and float((ob - torch.cat(one)).abs().max()) < 1e-5 * max(float(ob.abs().max()), 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 13])
@pytest.mark.parametrize("fill", [0.0, -1.0])
def test_paint_is_bit_exact(C, fill):
    from camouflage_multimodal_amd import paint_regions
    segs, rmap, off = _paint_batch()
    val = np.random.RandomState(C).standard_normal((48, C)).astype(np.float32)
    val[3, 0] = -0.0; val[4, 0] = 1e-42                                      # (bits, not values: a negative zero and a subnormal)
    st, rt, vt = torch.from_numpy(segs.copy()).cuda(), torch.from_numpy(rmap.copy()).cuda(), torch.from_numpy(val).cuda()
    got = paint_regions(vt, st, rt, [int(v) for v in off], fill=fill)
    want = R.paint(val, segs, rmap, off, fill)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, C, 33, 70)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert got[0, 0, 0, 0] == fill and got[0, C - 1, 5, 5] == fill           # label == label_bound, negative label
    assert np.array_equal(_bits(paint_regions(vt, st, rt, torch.from_numpy(off.copy()), fill=fill).cpu().numpy()), _bits(want))   # offsets as a tensor
    for i in range(3):                                                       # the single-image form equals the batch's slice
        single = paint_regions(vt[off[i]:off[i + 1]], st[i], rt[i], None, fill=fill)
        assert tuple(single.shape) == (1, C, 33, 70) and torch.equal(single[0], got[i])
    if C == 1:
        assert torch.equal(paint_regions(vt[:, 0], st, rt, list(off), fill=fill), got)      # values [n] are one channel


@pytest.mark.gpu
def test_paint_256x256_with_500_regions():
    from camouflage_multimodal_amd import paint_regions
    segs = np.stack([FO.voronoi_segments(256, 256, 500, 7), FO.voronoi_segments(256, 256, 480, 8)]).astype(np.int32)
    rmap, off = R.region_map_of(segs, 501)
    val = np.random.RandomState(2).uniform(0, 1, (int(off[-1]), 3)).astype(np.float32)
    got = paint_regions(torch.from_numpy(val).cuda(), torch.from_numpy(segs).cuda(), torch.from_numpy(rmap).cuda(), list(off))
    assert int(off[-1]) == 980 and np.array_equal(_bits(got.cpu().numpy()), _bits(R.paint(val, segs, rmap, off)))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("H,W", [(1, 1), (33, 70), (256, 256)])
def test_counts_are_exact(H, W, N):
    from camouflage_multimodal_amd import segmentation_counts
    rs = np.random.RandomState(H + N)
    maps = rs.uniform(0, 1, (N, 3, H, W)).astype(np.float32)
    sel = rs.uniform(size=(N, H, W))
    maps[:, 1][sel < 0.1] = 0.5                                              # the threshold exactly: not positive
    maps[:, 1][(sel >= 0.1) & (sel < 0.15)] = 0.0
    maps[:, 1][(sel >= 0.15) & (sel < 0.2)] = 1.0
    gt = rs.choice(np.array([0, 127, 128, 255], np.uint8), (N, H, W))
    if N == 5:
        maps[3, 1] = 0.0; gt[3] = 127                                        # all empty
        maps[4, 1] = 1.0; gt[4] = 255                                        # all full
    want = R.counts(maps[:, 1], gt, 0.5)
    assert (want[:, :4].sum(1) == H * W).all()
    mt, gtt = torch.from_numpy(maps).cuda(), torch.from_numpy(gt).cuda()
    got = segmentation_counts(mt[:, 1], gtt, 0.5)                            # strided: channel 1 of [N, 3, H, W], read in place
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (N, 5)
    print(f"{N} x {H} x {W}: counts {got.cpu().numpy().tolist()[:2]}")
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(segmentation_counts(mt[:, 1], gtt, 0.5), got)         # two calls: the same bytes
    assert torch.equal(segmentation_counts(mt[:, 1].contiguous(), gtt, 0.5), got)
    for i in range(N):                                                       # a batch gives the rows of its images one by one
        assert torch.equal(segmentation_counts(mt[i, 1], gtt[i], 0.5)[0], got[i])
    if N == 5:
        assert got[3].tolist() == [0, 0, 0, H * W, 0] and got[4].tolist() == [H * W, 0, 0, 0, 0]
        assert torch.equal(segmentation_counts(mt[:, 1], gtt > 127, 0.5), got)    # a bool mask
    other = R.counts(maps[:, 0], gt, 0.25)
    assert np.array_equal(segmentation_counts(mt[:, 0], gtt, 0.25).cpu().numpy(), other)


@pytest.mark.gpu
def test_detect_camouflage_batch_end_to_end():
    import slic_ref as SR
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage, detect_camouflage_batch
    torch.manual_seed(3)
    m = RegionGraphGNN().cuda().eval()
    for bn in (m.bn1, m.bn2, m.bn3, m.bn4):
        bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    H, W = 96, 80
    imgs = np.stack([SR.noise_image(H, W, 40 + i) for i in range(3)])
    yy, xx = np.mgrid[:H, :W]
    gt = np.zeros((3, H, W), np.uint8)
    gt[0][(yy - 40) ** 2 + (xx - 30) ** 2 < 20 ** 2] = 255                   # a disc
    gt[2][(yy - 70) ** 2 + (xx - 60) ** 2 < 12 ** 2] = 200                   # (the second image's mask stays empty)
    out = detect_camouflage_batch(m, torch.from_numpy(imgs).cuda(), torch.from_numpy(gt).cuda(), n_segments=60, threshold=0.5)
    g = out["graphs"]
    n = g.node_offsets[-1]
    assert tuple(out["prob_maps"].shape) == (3, 3, H, W) and out["mask"].dtype == torch.bool and tuple(out["mask"].shape) == (3, H, W)
    assert tuple(out["node_probs"].shape) == (n, 3) and tuple(out["segments"].shape) == (3, H, W) and g.num_graphs == 3 and n >= 3 * 20
    maps, probs = out["prob_maps"].cpu().numpy(), out["node_probs"].cpu().numpy()
    segs, rmap = out["segments"].cpu().numpy(), out["region_map"].cpu().numpy()
    # the maps are the call's own node probabilities painted through its own label maps, bit for bit; every pixel has a region
    assert np.array_equal(_bits(maps), _bits(R.paint(probs, segs, rmap, np.asarray(g.node_offsets))))
    assert np.array_equal(_bits(maps), _bits(R.paint(probs, segs, rmap, np.asarray(g.node_offsets), fill=-1.0)))
    assert np.array_equal(out["mask"].cpu().numpy(), maps[:, 0] > np.float32(0.5))
    # the metrics are the header's ratios of the counts of the call's own maps
    want = R.counts(maps[:, 0], gt, 0.5)
    assert len(out["metrics"]) == 3
    for i, got in enumerate(out["metrics"]):
        ref = R.ratios(want[i], H, W)
        print(f"image {i}: counts {want[i].tolist()}, iou {ref['iou']:.4f}, mae {ref['mae']:.4f}")
        for k, v in ref.items():
            assert got[k] == v, (i, k, got[k], v)
        assert [got[k] for k in ("tp", "fp", "fn", "tn")] == want[i, :4].tolist()
    # the batch's node probabilities are those of every image's graph alone, at the GNN's batch bound
    alone = torch.cat([m.node_probabilities(d) for d in g.graphs()])
    assert float((alone - out["node_probs"]).abs().max()) < 1e-5 * max(float(alone.abs().max()), 1.0)
    assert (probs > 0).all() and (probs < 1).all()
    # without masks: no metrics; the single-image wrapper is the batch of one
    assert "metrics" not in detect_camouflage_batch(m, torch.from_numpy(imgs).cuda(), n_segments=60)
    one = detect_camouflage(m, torch.from_numpy(imgs[1]).cuda(), torch.from_numpy(gt[1]).cuda(), n_segments=60)
    assert tuple(one["prob_maps"].shape) == (1, 3, H, W) and torch.equal(one["segments"][0], out["segments"][1]) and len(one["metrics"]) == 1
    assert float((one["prob_maps"][0] - out["prob_maps"][1]).abs().max()) < 1e-5


@pytest.mark.gpu
def test_attention_to_pixels():
    from camouflage_multimodal_amd import attention_to_pixels
    segs, rmap, off = _paint_batch()
    rs = np.random.RandomState(9)
    attn = [rs.uniform(0, 1, (13, int(off[i + 1] - off[i]))).astype(np.float32) for i in range(3)]
    st, rt = torch.from_numpy(segs.copy()).cuda(), torch.from_numpy(rmap.copy()).cuda()
    got = attention_to_pixels([{"kg2rg": torch.from_numpy(a).cuda(), "rg2kg": None} if i == 1 else torch.from_numpy(a).cuda()
                               for i, a in enumerate(attn)], st, rt, list(off))
    want = R.paint(np.concatenate([a.T for a in attn]), segs, rmap, off)
    assert tuple(got.shape) == (3, 13, 33, 70)
    for c in range(13):                                                      # every category's heat map
        assert np.array_equal(_bits(got[:, c].cpu().numpy()), _bits(want[:, c])), c
