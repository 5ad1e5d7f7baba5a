"""The structure loss on the painted mask (include/camo_rg_pixel_loss.h) against tests/rg_pixel_loss_ref.py.

PARITY UNPINNED (the reference's trainer cannot be read here): the header is the definition.  The CPU tests hold the restatement to
torch's own avg_pool2d, its node form to the literal F3Net loss taken pixel by pixel through the paint (float64, 1e-12), and both
entries' argument checks to the header.  On the GPU

  * the node weights are integers: every element of node_w is compared for EXACT equality, on buffers between guard bands that were
    filled with garbage (tests/guarded.py through tests/raw_calls.py's Call / execute);
  * the six loss figures and all 32 gradients are held to float64 autograd of the PIXEL form by the project's bound,

        e = max|g - g64| / max(max|g64|, 1e-12)  <=  8 e32 + 2e-6,

    e32 being the same error of torch-CPU float32 autograd of the NODE form, computed in the same test.  The graphs, parameters and
    seeds are those of tests/test_rg_train.py's cases "real", "batch", "many" and "saturated" (and of tests/test_rg_train_drop.py's
    "real" for batch statistics and dropout): their flip-clear margins depend on neither targets nor loss, and are asserted on the
    reference again.  The label maps are synthetic, 33 x 70 or smaller.  The library is called directly (tests/rg_train_calls.py), its
    workspace and its 33 outputs between guard bands.
"""
import functools
import os

import numpy as np
import pytest
import torch

import rg_maps
import rg_pixel_loss_ref as PR
import rg_targets_ref as TG
import rg_train_bn_ref as BR
import rg_train_ref as TR
import test_rg_targets as TT
import test_rg_train as T0
import test_rg_train_drop as TD
from conftest import ROOT
from oracle import rg_features_oracle as FO
from raw_calls import Call, execute
from rg_train_calls import direct, refuse
from test_rg_train import NAMES, _bits, _csr_pair, _data, _err, _model, _targets

E_ARG, E_UNSUPPORTED = -1, -2
FIGURES = ("loss", "mask_loss", "instance_loss", "edge_loss", "wbce", "wiou")


# ---- label maps and ground truths ---------------------------------------------------------------------------------------------

def _runs(rs, H, W, k):
    """int32 [H, W]: k regions of unequal sizes, runs of the raster order with random cuts (k = 0: all zeros, to go with no region)."""
    if k == 0:
        return np.zeros((H, W), np.int32)
    cuts = np.sort(rs.choice(np.arange(1, H * W), k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    return np.searchsorted(cuts, np.arange(H * W), side="right").reshape(H, W).astype(np.int32)


def _bytes_mask(rs, N, H, W, k=3):
    """uint8 [N, H, W]: random discs, the bytes drawn from {0, 127} outside and {128, 255} inside."""
    pos = TT._blobs(rs, N, H, W, k) > 127
    pick = rs.uniform(size=pos.shape) < 0.5
    return np.where(pos, np.where(pick, 128, 255), np.where(pick, 127, 0)).astype(np.uint8)


def _disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _maps(name):
    """(segments int32 [N, H, W], region_map int32 [N, label_bound], node_off int32 [N + 1], gt uint8 [N, H, W]) for the nodes of
    tests/test_rg_train.py's case of that name; read-only."""
    rs = np.random.RandomState(77)
    if name == "real":                        # one image of 23 regions, a disc
        seg = FO.voronoi_segments(33, 70, 23, 5)[None]
        gt = _disc(33, 70, 15, 30, 11)[None]
    elif name == "batch":                     # 23, 1 and 40 regions; a disc, a full and an empty ground truth
        seg = np.stack([FO.voronoi_segments(33, 70, 23, 5), np.ones((33, 70), np.int32), _runs(rs, 33, 70, 40)])
        gt = np.stack([_disc(33, 70, 15, 30, 11), np.full((33, 70), 255, np.uint8), np.zeros((33, 70), np.uint8)])
    elif name == "many":                      # one image of 1049 regions: more nodes than a block has threads
        seg = _runs(rs, 33, 70, 1049)[None]
        gt = _bytes_mask(rs, 1, 33, 70)
    elif name == "many51":                    # the same 1049 nodes as 51 images of 12 x 14, one of them without a node
        seg = np.stack([_runs(rs, 12, 14, k) for k in MANY51])
        gt = _bytes_mask(rs, 51, 12, 14, k=2)
    else:
        raise KeyError(name)
    lb = int(seg.max()) + 1
    rmap, off = TG.compact_region_map(seg, lb)
    if name == "many51":
        empty = MANY51.index(0)
        rmap[empty] = -1                      # its label 0 has no region
        off = np.concatenate([[0], np.cumsum(MANY51)]).astype(np.int32)
    out = (seg.astype(np.int32), rmap, off.astype(np.int32), gt)
    for a in out:
        a.setflags(write=False)
    return out


_S51 = T0._sizes("many")
MANY51 = (_S51[0] + _S51[1], 0) + tuple(_S51[2:])        # 51 images again: the first two graphs as one image, then an image without a node


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_header_symbols_binding_and_abi_version():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_rg_pixel_loss.h")).read()
    assert _lib.symbols("camo_rg_pixel_loss.h") == ("camo_rg_pixel_weights", "camo_rg_loss_backward_pixel")
    assert "PARITY UNPINNED" in hdr and "F3Net" in hdr and "TWO launches" in hdr and "No workspace" in hdr
    assert f"#define CAMO_RGPL_MAX_RADIUS {_lib.RGPL_MAX_RADIUS} " in hdr and f"#define CAMO_RGPL_MAX_GAIN {_lib.RGPL_MAX_GAIN} " in hdr
    assert _lib.ABI_VERSION == 13 and _lib.lib().camo_abi_version() == 13


@pytest.mark.parametrize("shape", [(33, 70), (5, 7), (1, 1)])
def test_q_over_k_is_torchs_weit(shape):
    rs = np.random.RandomState(0)
    gt = _bytes_mask(rs, 2, *shape, k=2)
    g = torch.from_numpy((gt > 127).astype(np.float64))
    for radius in (0, 1, 15, 31):
        for gain in (0, 5, 16):
            q, gi, K = PR.pixel_q(gt, radius, gain)
            assert K == (2 * radius + 1) ** 2 and np.array_equal(gi, (gt > 127)) and q.dtype == np.int64 and q.min() >= K
            weit = 1 + gain * torch.abs(torch.nn.functional.avg_pool2d(g[:, None], 2 * radius + 1, 1, radius)[:, 0] - g)
            assert np.abs(q / K - weit.numpy()).max() <= 1e-12, (shape, radius, gain)


def _both_forms(seg, rmap, off, gt, z, radius, gain):
    node_w = PR.node_weights(seg, rmap, off, gt, radius, gain)
    out = []
    for form in (lambda t: PR.pixel_form(t, seg, rmap, off, gt, radius, gain), lambda t: PR.node_form(t, node_w, off, radius)):
        t = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        figs = form(t)
        g, = torch.autograd.grad(figs[0], t, allow_unused=True)
        out.append(([float(v.detach()) for v in figs], np.zeros_like(z) if g is None else g.numpy()))
    return node_w, out


@pytest.mark.parametrize("shape, regions", [((33, 70), 23), ((5, 7), 4)])
def test_the_node_form_is_the_literal_loss_on_the_painted_map(shape, regions):
    """Loss and d/dz of the two forms agree to 1e-12 relative in float64; 5 x 7 is smaller than the 31 x 31 window.  Two images, so the
    mean over the images is in it; and the header's closed-form gradient is autograd's."""
    rs = np.random.RandomState(1)
    seg = np.stack([_runs(rs, *shape, regions), _runs(rs, *shape, regions)])
    rmap, off = TG.compact_region_map(seg, regions)
    gt = _bytes_mask(rs, 2, *shape, k=2)
    assert 0 < (gt > 127).sum() < gt.size
    z = rs.normal(0, 2, size=2 * regions)
    for radius, gain in ((15, 5), (1, 16), (0, 0)):
        node_w, ((fp, gp), (fn, gn)) = _both_forms(seg, rmap, off, gt, z, radius, gain)
        for a, b in zip(fp, fn):
            assert abs(a - b) <= 1e-12 * abs(a), (radius, gain, fp, fn)
        assert np.abs(gp - gn).max() <= 1e-12 * np.abs(gp).max() and np.abs(gp).max() > 1e-4
        assert np.abs(PR.node_gradient(z, node_w, off, radius) - gp).max() <= 1e-12 * np.abs(gp).max()
        assert abs(fp[0] - (fp[1] + fp[2])) <= 1e-15 and fp[1] > 0 and 0 < fp[2] < 1


def test_radius_zero_gives_the_counts():
    seg, rmap, off, gt, _ = TT._excluded_case()
    counts = TG.node_counts(seg, rmap, off, gt)
    for gain in (0, 5, 16):
        assert np.array_equal(PR.node_weights(seg, rmap, off, gt, 0, gain), counts[:, :2])
    n = int(off[2]) - 9                                               # n_nodes below node_off[N]: the rows below it do not change
    assert np.array_equal(PR.node_weights(seg, rmap, off, gt, 15, 5, n_nodes=n), PR.node_weights(seg, rmap, off, gt, 15, 5)[:n])


def test_conventions_empty_and_full_ground_truth_and_an_image_without_a_node():
    seg, rmap, off, gt = _maps("batch")
    node_w = PR.node_weights(seg, rmap, off, gt)
    K = 31 * 31
    full, empty = slice(off[1], off[2]), slice(off[2], off[3])
    # a full mask: S < K near the border (zero padding), so q > K there; B = A.  An empty one: q = K everywhere, B = 0.
    assert node_w[full, 0].sum() > K * 33 * 70 and np.array_equal(node_w[full, 0], node_w[full, 1])
    assert node_w[empty, 0].sum() == K * 33 * 70 and not node_w[empty, 1].any()
    z = np.random.RandomState(2).normal(0, 1, size=int(off[3]))
    _, ((fp, gp), (fn, gn)) = _both_forms(seg, rmap, off, gt, z, 15, 5)
    assert all(abs(a - b) <= 1e-12 * abs(a) for a, b in zip(fp, fn)) and np.abs(gp - gn).max() <= 1e-12 * np.abs(gp).max()
    # an image without a node is left out of the mean: 51 images, 50 of them counted
    seg, rmap, off, gt = _maps("many51")
    i = MANY51.index(0)
    assert off[i] == off[i + 1] and len(off) == 52 and off[-1] == 1049
    z = np.random.RandomState(3).normal(0, 1, size=1049)
    node_w, ((fp, gp), (fn, gn)) = _both_forms(seg, rmap, off, gt, z, 15, 5)
    assert all(abs(a - b) <= 1e-12 * abs(a) for a, b in zip(fp, fn)) and np.abs(gp - gn).max() <= 1e-12 * np.abs(gp).max()
    keep = [k for k in range(51) if k != i]
    per = [PR.node_form(torch.tensor(z[off[k]:off[k + 1]]), node_w[off[k]:off[k + 1]], [0, off[k + 1] - off[k]])[0] for k in keep]
    assert abs(float(sum(per)) / 50 - fn[0]) <= 1e-12
    # no image left: zero loss, zero gradient
    none = PR.node_form(torch.tensor(z, requires_grad=True), np.zeros_like(node_w), off)
    assert [float(v.detach()) for v in none] == [0.0, 0.0, 0.0] and not PR.node_gradient(z, np.zeros_like(node_w), off).any()
    # offsets out of range are clamped and a decreasing pair is an empty image
    a = PR.node_form(torch.tensor(z), node_w, [-7, 24, 4000, 30])
    b = PR.node_form(torch.tensor(z), node_w, [0, 24, 1049, 1049])
    assert [float(v) for v in a] == [float(v) for v in b]


def test_argument_checks_of_the_weights_entry_match_the_header():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    fake = 0x1000                                    # never dereferenced: every check runs on the host before any launch
    names = ("segments", "region_map", "node_off", "gt_mask", "node_w")

    def call(N=2, H=70, W=33, label_bound=64, n_nodes=50, radius=15, gain=5, null=()):
        p = {k: (None if k in null else fake) for k in names}
        rc = L.camo_rg_pixel_weights(p["segments"], p["region_map"], p["node_off"], p["gt_mask"], N, H, W, label_bound, n_nodes, radius, gain,
                                     p["node_w"], None)
        return rc, L.camo_last_error()

    for kw, word in ((dict(N=0), b"N"), (dict(H=0), b"H"), (dict(W=-1), b"W"), (dict(label_bound=0), b"label_bound"),
                     (dict(label_bound=4097), b"label_bound"), (dict(n_nodes=0), b"n_nodes"),
                     (dict(N=1, H=8193, W=8192), b"CAMO_RGB_MAX_IMAGE_PIXELS"), (dict(N=3, H=8192, W=8192), b"CAMO_RGB_MAX_PIXELS"),
                     (dict(radius=-1), b"radius"), (dict(radius=32), b"radius"), (dict(gain=-1), b"gain"), (dict(gain=17), b"gain")):
        rc, msg = call(**kw)
        assert rc == E_ARG and word in msg, (kw, rc, msg)
    for name in names:
        rc, msg = call(null=(name,))
        assert rc == E_ARG and name.encode() in msg, (name, rc, msg)


def test_argument_checks_of_the_loss_entry_match_the_header():
    def call(**kw):                                  # fake pointers: every check runs on the host before any launch
        return refuse("camo_rg_loss_backward_pixel", hidden=32, heads=2, **kw)[:2]

    rc, msg = call(nc=3)
    assert rc == E_UNSUPPORTED and b"num_classes == 2" in msg
    for kw, word in ((dict(n_images=0), b"n_images"), (dict(radius=-1), b"radius"), (dict(radius=32), b"radius"), (dict(w_pixel=-0.5), b"w_pixel"),
                     (dict(w_pixel=float("inf")), b"w_pixel"), (dict(w_pixel=float("nan")), b"w_pixel"), (dict(null="node_w"), b"node_w"),
                     (dict(null="node_off"), b"node_off")):
        rc, msg = call(**kw)
        assert rc == E_ARG and word in msg, (kw, rc, msg)
    # what camo_rg_loss_backward_drop refuses is refused as it refuses it
    assert call(ws_bytes=1024)[0] == -3 and call(null="x")[0] == E_ARG and call(mode=2)[0] == E_ARG and call(rates=(1.0, 0.0, 0.0))[0] == E_ARG


def test_cpu_tensors_and_bad_options_raise():
    from camouflage_multimodal_amd import RegionGraphData, RegionGraphFineTuner, RegionGraphGNN
    from camouflage_multimodal_amd._lib import CamoError
    from camouflage_multimodal_amd.rg_finetune import pixel_loss_weights, prepare_finetune_batch
    seg = torch.zeros(1, 8, 8, dtype=torch.int32)
    with pytest.raises(CamoError):
        pixel_loss_weights(seg, torch.zeros(1, 1, dtype=torch.int32), [0, 1], torch.zeros(1, 8, 8, dtype=torch.uint8))
    c = T0._case("isolated")
    m = RegionGraphGNN()
    data = RegionGraphData(torch.from_numpy(c["x"].copy()), torch.from_numpy(c["ei"].copy()), torch.from_numpy(c["ew"].copy())[:, None])
    t = [torch.from_numpy(c[k].copy()) for k in ("mt", "it", "et")]
    node_w = torch.ones(c["n"], 2, dtype=torch.int64)
    with pytest.raises(CamoError):
        m.loss_and_gradients(data, *t, pixel=(node_w, [0, c["n"]], 15, 1.0))
    for bad in ((node_w, [0, c["n"]], 32, 1.0), (node_w, [0, c["n"]], 15, -1.0), (node_w, [0, c["n"]], 15, float("nan"))):
        with pytest.raises(ValueError, match="pixel loss"):                     # before any device work
            m.loss_and_gradients_csr(data.x, (None,) * 3, (None,) * 3, *t, pixel=bad)
    assert all(p.grad is None for p in m.parameters())
    for kw in (dict(pixel_loss=-1.0), dict(pixel_loss=float("nan")), dict(pixel_loss=1.0, pixel_radius=32), dict(pixel_loss=1.0, pixel_gain=17)):
        with pytest.raises(ValueError, match="pixel_"):
            RegionGraphFineTuner(RegionGraphGNN(hidden_channels=32, heads=2), **kw)
    with pytest.raises(ValueError, match="pixel_loss must be"):
        prepare_finetune_batch(torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, dtype=torch.uint8), pixel_loss={"window": 3})
    tuner = RegionGraphFineTuner(RegionGraphGNN(hidden_channels=32, heads=2), pixel_loss=1.0)
    with pytest.raises(CamoError):
        tuner.step_from_images(torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, dtype=torch.uint8))


@pytest.mark.parametrize("name", ["real", "batch", "many", "saturated"])
def test_cases_stay_clear_of_a_relu_flip_and_the_maps_are_what_they_claim(name):
    c = _loss_case(name, 1.0)
    assert c["margin"] > TR.FLIP_MARGIN and abs(c["margin"] - T0._case(name)["margin"]) <= 1e-9      # (neither targets nor loss reach the forward)
    seg, rmap, off, gt = c["maps"]
    assert seg.shape[1:] == (33, 70) and off[-1] == c["n"] and np.diff(off).tolist() == list(c["sizes"] if name == "batch" else (c["n"],))
    assert (c["node_w"][:, 0] > 0).all() and c["node_w"][:, 0].sum() >= 31 * 31 * seg.size
    if name == "batch":
        assert not (gt[2] > 127).any() and (gt[1] > 127).all()
    if name in ("many", "saturated"):
        assert c["n"] == 1049 > 1024 and len(off) == 2
    if name == "saturated":                                            # in fp32 1 - p rounds to 1 and p (1 - p) is lost beside A p - B
        z = c["z64"]
        p32 = (1.0 / (1.0 + np.exp(-z.astype(np.float32)))).astype(np.float32)
        assert np.abs(z).min() > 40 and (np.float32(1) - p32 == 1).all() and (p32 * (1 - p32) < 1e-17).all()


# ---- GPU, the weights -----------------------------------------------------------------------------------------------------

def _weights_call(seg, rmap, off, gt, radius, gain, n_nodes=None):
    from camouflage_multimodal_amd import _lib
    L, (N, H, W) = _lib.lib(), seg.shape
    n = int(off[-1]) if n_nodes is None else int(n_nodes)
    ins = {"segments": np.asarray(seg, np.int32), "region_map": np.asarray(rmap, np.int32), "node_off": np.asarray(off, np.int32),
           "gt": np.asarray(gt, np.uint8)}
    stream = torch.cuda.current_stream().cuda_stream
    return Call({"node_w": ((n, 2), np.int64)}, 0,
                lambda p, w, nb: L.camo_rg_pixel_weights(p["segments"], p["region_map"], p["node_off"], p["gt"], N, H, W, rmap.shape[1], n, radius,
                                                         gain, p["node_w"], stream), ins)


def _check_weights(seg, rmap, off, gt, radius, gain, n_nodes=None, fill=0xA5, skew=0, tag=""):
    want = PR.node_weights(seg, rmap, off, gt, radius, gain, n_nodes)
    got = execute(_weights_call(seg, rmap, off, gt, radius, gain, n_nodes), fill, skew=skew)["node_w"]
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), (tag, radius, gain, np.argwhere(got != want)[:5].tolist())
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("shape, N", [((1, 1), 1), ((5, 7), 5), ((33, 70), 5)])
def test_weights_at_every_radius_and_gain(shape, N):
    """Images smaller than the window, of one pixel, and 33 x 70 (two tile rows, three tile columns, none of them full); bytes 0, 127,
    128 and 255; the output pre-filled with 0xA5, 0xFF and 0x7F and begun 8 bytes past a 256-byte boundary."""
    rs = np.random.RandomState(4)
    H, W = shape
    k = min(H * W, 9)
    seg = np.stack([_runs(rs, H, W, k) for _ in range(N)])
    rmap, off = TG.compact_region_map(seg, k)
    gt = _bytes_mask(rs, N, H, W, k=2) if H * W > 1 else np.full((1, 1, 1), 128, np.uint8)
    assert set(np.unique(gt)) <= {0, 127, 128, 255}
    fills = (0xA5, 0xFF, 0x7F)
    for j, (radius, gain) in enumerate((r, g) for r in (0, 1, 15, 31) for g in (0, 5, 16)):
        want = _check_weights(seg, rmap, off, gt, radius, gain, fill=fills[j % 3], skew=8 * (j % 2), tag=str(shape))
        assert want[:, 0].sum() >= (2 * radius + 1) ** 2 * N * H * W


@functools.lru_cache(maxsize=None)
def _large():
    rs = np.random.RandomState(6)
    seg = FO.voronoi_segments(256, 256, 500, 9)[None]
    rmap, off = TG.compact_region_map(seg, 512)
    assert 480 <= off[1] <= 500
    return seg, rmap, off, _bytes_mask(rs, 1, 256, 256, k=5)


@pytest.mark.gpu
@pytest.mark.parametrize("radius, gain", [(15, 5), (31, 16)])
def test_weights_of_a_256_image_with_500_regions(radius, gain):
    seg, rmap, off, gt = _large()
    want = _check_weights(seg, rmap, off, gt, radius, gain, tag="256 x 256")
    assert want[:, 0].sum() > (2 * radius + 1) ** 2 * 256 * 256 and 0 < want[:, 1].sum() < want[:, 0].sum()


@pytest.mark.gpu
def test_weights_with_excluded_pixels_and_rows_past_n_nodes():
    """A label equal to label_bound, a negative one, 2^31 - 1, a region_map of -1 and a node no pixel carries; then n_nodes below
    node_off[N]: the pixels of the nodes past it take no part and nothing past row n_nodes is written."""
    seg, rmap, off, gt, _ = TT._excluded_case()
    assert (seg == rmap.shape[1]).any() and (seg < 0).any() and (rmap[0, 7] == -1)
    want = _check_weights(seg, rmap, off, gt, 15, 5, tag="excluded")
    assert want[off[2] - 1].tolist() == [0, 0] and (want[:off[2] - 1, 0] > 0).all()
    n = int(off[2]) - 9
    _check_weights(seg, rmap, off, gt, 15, 5, n_nodes=n, fill=0x7F, tag="n_nodes below node_off[N]")
    _check_weights(seg, rmap, off, gt, 0, 16, tag="the counts")


@pytest.mark.gpu
def test_weights_with_more_nodes_than_slots_in_a_tile_and_a_label_in_two_tiles():
    rs = np.random.RandomState(8)
    _, seg, _ = rg_maps.case("perm64")                                 # every pixel its own region: 1024 nodes in a tile, 960 past the table
    assert rg_maps.most_labels_in_a_tile(seg) == 1024 > 64
    rmap, off = TG.compact_region_map(seg[None], 4096)
    want = _check_weights(seg[None], rmap, off, _bytes_mask(rs, 1, 64, 64), 15, 5, tag="perm64")
    assert (want[:, 0] >= 961).all()
    _, seg, _ = rg_maps.case("split")                                  # label 3 lies in the tiles at (0, 0) and at (32, 32)
    ys, xs = np.nonzero(seg == rg_maps.SPLIT_LABEL)
    assert len({(y // 32, x // 32) for y, x in zip(ys, xs)}) >= 2
    rmap, off = TG.compact_region_map(seg[None], 16)
    _check_weights(seg[None], rmap, off, _bytes_mask(rs, 1, 70, 70), 15, 5, tag="split")


@pytest.mark.gpu
def test_weights_of_a_batch_are_its_images_and_two_calls_give_the_same_bytes():
    rs = np.random.RandomState(11)
    seg = np.stack([TT._blocks(1, 45, 50, b)[0] for b in (5, 9, 25, 7, 50)])
    rmap, off = TG.compact_region_map(seg, 128)
    gt = _bytes_mask(rs, 5, 45, 50)
    whole = _check_weights(seg, rmap, off, gt, 15, 5, tag="batch")
    call = _weights_call(seg, rmap, off, gt, 15, 5)
    other = _weights_call(seg, rmap, off, gt[::-1].copy(), 31, 16)
    again = execute(call, 0xFF, before=(other, call))["node_w"]       # on what two earlier calls left in the accumulator
    assert again.tobytes() == whole.tobytes()
    for i in range(5):
        got = execute(_weights_call(seg[i:i + 1], rmap[i:i + 1], [0, off[i + 1] - off[i]], gt[i:i + 1], 15, 5), 0xA5)["node_w"]
        assert got.tobytes() == whole[off[i]:off[i + 1]].tobytes(), i


@pytest.mark.gpu
def test_the_wrapper_returns_the_weights_on_the_device():
    from camouflage_multimodal_amd.rg_finetune import pixel_loss_weights
    seg, rmap, off, gt = _maps("batch")
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (seg, rmap, gt)]
    got = pixel_loss_weights(dev[0], dev[1], [int(v) for v in off], dev[2])
    assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), PR.node_weights(seg, rmap, off, gt))
    one = pixel_loss_weights(dev[0][0], dev[1][0], [0, int(off[1])], dev[2][0] > 127, radius=1, gain=16)        # [H, W], a bool mask
    assert np.array_equal(one.cpu().numpy(), PR.node_weights(seg[:1], rmap[:1], off[:2], gt[:1], 1, 16))


# ---- GPU, loss and gradients ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loss_case(name, w_pixel, weights=(1.0, 1.0, 1.0), maps=None, drop_key=None):
    """Inputs and both CPU references of a case, computed once; never written to.  l64 / g64: float64 autograd of the pixel form;
    l32 / g32: float32 autograd of the node form.  `drop_key`: (mode, rates, seed) on tests/test_rg_train_drop.py's inputs instead."""
    if drop_key is None:
        c = dict(T0._case(name))
        mode, rates, seed = 0, (0.0, 0.0, 0.0), 0
    else:
        mode, rates, seed = drop_key
        c = dict(TD._inputs(name, mode))
    seg, rmap, off, gt = _maps(maps or ("many" if name == "saturated" else name))
    node_w = PR.node_weights(seg, rmap, off, gt)
    node_w.setflags(write=False)
    args = (c["p"], c["x"], c["ei"], c["ew"], c["mt"], c["it"], c["et"], c["heads"], c["nc"])
    kw = dict(weights=weights, rates=rates, seed=seed, batch=bool(mode))
    zs = []
    c["l64"], c["g64"], c["margin"] = PR.loss_and_grads(*args, lambda z: (zs.append(z.detach().numpy()), PR.pixel_form(z, seg, rmap, off, gt))[1],
                                                        w_pixel, **kw)
    c["l32"], c["g32"], _ = PR.loss_and_grads(*args, lambda z: PR.node_form(z, node_w, off), w_pixel, dtype=torch.float32, **kw)
    c.update(maps=(seg, rmap, off, gt), node_w=node_w, w_pixel=w_pixel, weights=weights, mode=mode, rates=rates, seed=seed, z64=zs[0])
    return c


def _direct(m, c, d, pair, w_pixel=None, node_w=None, node_off=None, entry="pixel"):
    """camo_rg_loss_backward_pixel (or _drop: `entry`) called directly through rg_train_calls.direct, which checks the guards round the
    workspace and every output and that every output element was written.  Returns (loss, the 32 gradients, batch_stats or None, the
    eight running statistics the call updated or None); the model's own are not touched."""
    own = None
    if entry == "pixel":
        nw = torch.from_numpy(np.array(c["node_w"] if node_w is None else node_w)).cuda()
        no = torch.from_numpy(np.array(c["maps"][2] if node_off is None else node_off, np.int32)).cuda()
        own = (nw, no, PR.RADIUS, c["w_pixel"] if w_pixel is None else w_pixel)
    got = direct("camo_rg_loss_backward_" + entry, m, d.x, pair, _targets(c), weights=c.get("weights", (1.0, 1.0, 1.0)), mode=c.get("mode", 0),
                 rates=c.get("rates", (0.0, 0.0, 0.0)), seed=c.get("seed", 0), momentum=BR.MOMENTUM, pixel=own)
    return got.loss, got.grads, got.bs, got.run


def _hold(c, loss6, grads, tag, skip=()):
    """The six figures and every gradient within 8 e32 + 2e-6 of float64 autograd of the pixel form; prints the largest e and e32."""
    worst, worst32 = 0.0, 0.0
    got = dict(zip(FIGURES, loss6), **{k: g for k, g in zip(NAMES, grads)})
    want64 = dict(zip(FIGURES, c["l64"]), **c["g64"])
    want32 = dict(zip(FIGURES, c["l32"]), **c["g32"])
    for k in FIGURES + tuple(NAMES):
        if k in skip:
            assert not _bits(got[k]).any(), (tag, k)                  # batch statistics: the conv-bias gradients are +0.0f bit for bit
            continue
        assert np.shape(got[k]) == np.shape(want64[k]), k
        e, e32 = _err(got[k], want64[k]), _err(want32[k], want64[k])
        print(f"{tag} {k}: e {e:.3g} e32 {e32:.3g}")
        worst, worst32 = max(worst, e), max(worst32, e32)
        assert e <= 8 * e32 + 2e-6, (tag, k, e, e32)
    print(f"{tag}: largest e {worst:.3g}, largest e32 {worst32:.3g}")


def _run_case(c, tag, **kw):
    assert c["margin"] > TR.FLIP_MARGIN                                # on the CPU reference, before the device is looked at
    m, d = _model(c).train(), _data(c)
    pair = _csr_pair(c, d)             # ONE pair for a test: the device builder leaves a row's edges in no particular order
    loss, grads, bs, run = _direct(m, c, d, pair, **kw)
    loss6 = loss.cpu().numpy().tolist()
    _hold(c, loss6, [g.cpu().numpy() for g in grads], tag, skip=TD.BIAS_NAMES if c["mode"] else ())
    assert abs(c["l64"][0] - (c["weights"][0] * c["l64"][1] + c["weights"][1] * c["l64"][2] + c["weights"][2] * c["l64"][3]
                              + c["w_pixel"] * (c["l64"][4] + c["l64"][5]))) <= 1e-12
    return m, d, pair, loss, grads, bs, run


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["real", "batch", "many", "saturated"])
def test_figures_and_gradients_match_float64_autograd_of_the_pixel_form(name):
    c = _loss_case(name, 1.0)
    _run_case(c, name)
    assert min(np.abs(c["g64"][k]).max() for k in ("fc_mask_1.weight", "fc_mask_2.weight", "conv1.lin.weight")) > 0


@pytest.mark.gpu
def test_an_image_may_be_empty_and_offsets_are_clamped():
    """"many" cut into 51 images with one that has no node; then the same call with offsets below 0, past N and decreasing, which the
    kernel clamps: the bytes of the call on the clamped offsets."""
    c = _loss_case("many", 1.0, maps="many51")
    assert len(c["maps"][2]) == 52 and 0 in np.diff(c["maps"][2])
    m, d, pair, loss, grads, _, _ = _run_case(c, "many as 51 images")
    wild = _direct(m, c, d, pair, node_off=[-7, 24, 4000, 30])
    tame = _direct(m, c, d, pair, node_off=[0, 24, 1049, 1049])
    assert np.array_equal(_bits(wild[0].cpu()), _bits(tame[0].cpu())) and all(TD._same(a, b) for a, b in zip(wild[1], tame[1]))
    none = _direct(m, c, d, pair, node_w=np.zeros_like(c["node_w"]))   # no image left: the pixel term is 0 with zero gradient
    old = _direct(m, c, d, pair, entry="drop")
    assert none[0][4:].tolist() == [0.0, 0.0] and TD._same(none[0][:4], old[0]) and all(TD._same(a, b) for a, b in zip(none[1], old[1]))


@pytest.mark.gpu
def test_the_mask_head_on_pixels_alone():
    c = _loss_case("real", 0.7, weights=(0.0, 1.0, 0.5))
    _run_case(c, "w_mask = 0")
    assert c["l64"][1] > 0 and np.abs(c["g64"]["fc_mask_2.weight"]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["real", "many"])
def test_zero_weight_is_the_existing_entry_byte_for_byte_and_two_calls_agree(name):
    c = _loss_case(name, 1.0)
    m, d = _model(c).eval(), _data(c)
    pair = _csr_pair(c, d)
    old = _direct(m, c, d, pair, entry="drop")
    new = _direct(m, c, d, pair, w_pixel=0.0)
    assert TD._same(new[0][:4], old[0]) and all(TD._same(a, b) for a, b in zip(new[1], old[1]))
    assert abs(float(new[0][4]) - c["l64"][4]) <= 1e-5 * c["l64"][4] and abs(float(new[0][5]) - c["l64"][5]) <= 1e-5      # still reported
    one, two = _direct(m, c, d, pair), _direct(m, c, d, pair)
    assert TD._same(one[0], two[0]) and all(TD._same(a, b) for a, b in zip(one[1], two[1]))
    assert not TD._same(one[1][NAMES.index("fc_mask_2.weight")], old[1][NAMES.index("fc_mask_2.weight")])


@pytest.mark.gpu
@pytest.mark.parametrize("key", [(1, (0.0, 0.0, 0.0), 0), (0, TD.ALL, TD.CONFIGS[("real", 0, TD.ALL)])], ids=["batch-statistics", "dropout"])
def test_batch_statistics_and_dropout_take_the_pixel_term_and_nothing_else_changes(key):
    c = _loss_case("real", 1.0, maps="real", drop_key=key)
    m, d, pair, loss, grads, bs, run = _run_case(c, "batch statistics" if key[0] else "dropout")
    old = _direct(_model(c).train(), c, d, pair, entry="drop")
    assert TD._same(loss[1:4], old[0][1:4])                            # the three existing terms
    if key[0]:                                                         # the batch statistics and the running statistics updated as without it
        assert TD._same(bs, old[2])
        for k, a, b in zip(TD.STAT_NAMES, run, old[3]):
            assert TD._same(a, b) and not np.array_equal(_bits(a.cpu()), _bits(c["p"][k])), k


@pytest.mark.gpu
def test_the_wrapper_is_the_direct_call():
    """loss_and_gradients_csr(pixel=...) gives the bytes of the direct call in all three modes, with the weights the device made;
    loss_and_gradients(pixel=...) returns the seven figures."""
    from camouflage_multimodal_amd.rg_finetune import pixel_loss_weights
    for key in (None, (1, (0.0, 0.0, 0.0), 0), (0, TD.ALL, 19)):
        c = _loss_case("real", 1.0, maps="real", drop_key=key)
        seg, rmap, off, gt = c["maps"]
        node_w = pixel_loss_weights(*[torch.from_numpy(np.array(a)).cuda() for a in (seg, rmap)], [int(v) for v in off],
                                    torch.from_numpy(np.array(gt)).cuda())
        assert np.array_equal(node_w.cpu().numpy(), c["node_w"])
        m, d = _model(c).train(), _data(c)
        pair = _csr_pair(c, d)
        want = _direct(_model(c).train(), c, d, pair)
        loss, grads = m.loss_and_gradients_csr(d.x, *pair, *_targets(c), batch_stats=bool(c["mode"]), dropout=c["rates"], seed=c["seed"],
                                               pixel=(node_w, [int(v) for v in off], PR.RADIUS, 1.0))
        assert loss.shape == (6,) and TD._same(loss, want[0]) and all(TD._same(a, b) for a, b in zip(grads, want[1]))
    c = _loss_case("real", 1.0)
    m, d = _model(c).eval(), _data(c)
    out = m.loss_and_gradients(d, *_targets(c), pixel=(node_w, torch.tensor([0, 23]), PR.RADIUS, 1.0))
    assert set(out) == {"loss", "mask_loss", "instance_loss", "edge_loss", "pixel_loss", "wbce", "wiou"}
    assert all(v.dim() == 0 and v.is_cuda for v in out.values()) and float(out["pixel_loss"]) == float(out["wbce"] + out["wiou"])
    assert all(p.grad is not None for p in m.trainable_parameters())
    assert set(m.loss_and_gradients(d, *_targets(c))) == {"loss", "mask_loss", "instance_loss", "edge_loss"}
