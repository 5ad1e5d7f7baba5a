"""Canny edge maps on the device (include/camo_canny.h) against tests/canny_ref.py.

PARITY UNPINNED (skimage absent): the checker restates the published scikit-image algorithm with scipy.ndimage.  CPU tests
hold the checker to scipy's own composition and to hand cases, and show that the end-to-end criterion holds for the checker
alone (float32 against float64); GPU tests hold the HIP kernels to the checker:

  gradients     |d| <= 2e-5 against float64.  Derived, not measured: inputs in [0, 1], each blur pass a convex sum of at most 17
                terms, Sobel weights summing to 8 -> 8 * 40 * 2^-24.
  decisions     exact: the float32 evaluation of decide() on the device's own gradients, every pixel.
  end to end    against float64, equal outside the excluded components (canny_ref.excluded_components, tau = 4 x the measured
                gradient error of that image); the excluded reference edge pixels are at most 10 % of the reference's, and the
                reference has at least 50 edge pixels -- except at 9 x 13, whose 7 x 11 interior cannot hold 50 pixels of
                one-pixel-wide lines under a 17-tap blur (its reference has 10): there it must have at least one.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import canny_ref as R
from conftest import ROOT
from raw_calls import BUILDERS, execute

GRAD_BOUND = 2e-5                         # 8 * 40 * 2^-24 = 1.9e-5, rounded up
EXCLUDED_CAP = 0.10
CASES = R.cases()
NAMES = tuple(CASES)


def _min_edges(name):
    return 1 if name == "9x13" else 50


@functools.lru_cache(maxsize=None)
def _ref64(name):
    """Per image of the case: (edges, (gi, gj, m), classes) in float64.  Computed once, never written to."""
    out = []
    for im in CASES[name]:
        e, g = R.canny(im, np.float64)
        out.append((e, g, R.classes(*g, 0.1, 0.2)))
    return out


def _end_to_end(name, k, other_edges, other_grad):
    """The end-to-end criterion for image k of a case; prints its figures before asserting."""
    e64, g64, c64 = _ref64(name)[k]
    err = max(float(np.abs(a - np.asarray(b, np.float64)).max()) for a, b in zip(g64, other_grad))
    ex = R.excluded_components(g64, c64, other_edges, 4 * err)
    share = float((e64 & ex).sum()) / max(int(e64.sum()), 1)
    wrong = int((e64 != other_edges)[~ex].sum())
    print(f"{name}[{k}]: gradient error {err:.3e}, reference edges {int(e64.sum())}, other edges {int(other_edges.sum())}, "
          f"excluded share {share:.4f}, mismatches outside {wrong}, mismatches in all {int((e64 != other_edges).sum())}")
    assert e64.sum() >= _min_edges(name)
    assert wrong == 0
    assert share <= EXCLUDED_CAP
    return err


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_stage_a_equals_the_scipy_composition():
    for name in NAMES:
        for im in CASES[name]:
            gray = R.luma(im)
            for a, b in zip(R.stage_a(gray, np.float64), R.stage_a_ndimage(gray)):
                assert np.abs(a - b).max() <= 1e-12
    assert len(R.gaussian_weights(2.0)) == 17 and abs(R.gaussian_weights(2.0).sum() - 1) < 1e-15


def test_hand_cases():
    H, W = 24, 32
    step = np.zeros((H, W)); step[:, 16] = 0.3; step[:, 17:] = 1.0           # (the 0.3 column breaks the tie of a symmetric step)
    e, _ = R.canny(R.grey_image(step))
    cols = np.nonzero(e.any(axis=0))[0]
    assert len(cols) == 1 and cols[0] in (16, 17)                            # one line, one pixel wide, at the step
    assert e[1:-1, cols[0]].all() and not e[0].any() and not e[-1].any() and not e[:, 0].any() and not e[:, -1].any()
    e, (gi, gj, m) = R.canny(R.grey_image(np.full((H, W), 0.7)))
    assert not e.any() and m.max() < 1e-12                                   # a constant image: the normalisation leaves no border gradient
    cls = np.zeros((9, 12), np.uint8)
    cls[2, 1:6] = 1                                                          # weak only: dropped
    cls[6, 1:5] = 1; cls[5, 5] = 2                                           # a weak run that touches a strong pixel only diagonally: kept
    cls[7, 9] = 2                                                            # a strong pixel alone
    want = np.zeros_like(cls, bool); want[6, 1:5] = True; want[5, 5] = True; want[7, 9] = True
    assert (R.hysteresis(cls) == want).all()


def test_float32_reference_meets_the_end_to_end_criterion():
    for name in NAMES:
        for k, im in enumerate(CASES[name]):
            e32, g32 = R.canny(im, np.float32)
            assert g32[2].dtype == np.float32
            assert _end_to_end(name, k, e32, g32) <= GRAD_BOUND


def test_binding_and_argument_checks_without_a_gpu():
    from camouflage_multimodal_amd import _lib, canny_edges
    hdr = open(os.path.join(ROOT, "include", "camo_canny.h")).read()
    assert "PARITY UNPINNED" in hdr
    assert _lib.ABI_VERSION == 13 and "#define CAMO_ABI_VERSION 13" in open(os.path.join(ROOT, "include", "camo_fusion.h")).read()
    L = _lib.lib()
    assert L.camo_abi_version() == 13
    need = L.camo_canny_workspace_bytes(2, 48, 64)
    assert need >= 2 * 48 * 64 * (12 + 1 + 4 + 1)
    assert L.camo_canny_workspace_bytes(0, 48, 64) == 0 and b"N >= 1" in L.camo_last_error()
    assert L.camo_canny_workspace_bytes(1, 48, 0) == 0
    assert L.camo_canny_workspace_bytes(64, 8192, 8192) == 0 and b"MAX_PIXELS" in L.camo_last_error()
    p = ctypes.c_void_p(0x1000)                                              # (never dereferenced: every check comes before any launch)

    def call(N=1, H=48, W=64, sigma=2.0, low=0.1, high=0.2, img=p, ws=p, nbytes=None, edges=p):
        return L.camo_canny(img, N, H, W, sigma, low, high, ws, L.camo_canny_workspace_bytes(1, 48, 64) if nbytes is None else nbytes,
                            edges, None, None)
    assert call(N=0) == -1 and call(H=0) == -1 and call(W=-3) == -1
    assert call(sigma=0.0) == -1 and b"sigma" in L.camo_last_error()
    assert call(sigma=float("nan")) == -1
    assert call(low=0.0) == -1 and b"low" in L.camo_last_error()
    assert call(low=0.3, high=0.2) == -1
    assert call(img=None) == -1 and call(ws=None) == -1 and call(edges=None) == -1 and b"null" in L.camo_last_error()
    assert call(sigma=9.0) == -2 and b"radius" in L.camo_last_error()
    assert call(nbytes=L.camo_canny_workspace_bytes(1, 48, 64) - 1) == -3 and b"camo_canny_workspace_bytes" in L.camo_last_error()
    assert L.camo_canny_hysteresis(None, 1, 8, 8, p, 1 << 20, p, None) == -1
    assert L.camo_canny_hysteresis(p, 1, 0, 8, p, 1 << 20, p, None) == -1
    assert L.camo_canny_hysteresis(p, 1, 8, 8, p, 16, p, None) == -3
    import torch
    with pytest.raises(_lib.CamoError):
        canny_edges(torch.zeros(8, 8, 3))
    with pytest.raises(_lib.CamoError):
        canny_edges(np.zeros((2, 8, 8, 3), np.float32), device="cpu")


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _device(name):
    """(edges bool [N, H, W], gradients fp32 [N, 3, H, W]) of a case's batch, as numpy; one call per case for all tests."""
    import torch
    from camouflage_multimodal_amd import canny_edges
    e, g = canny_edges(torch.from_numpy(CASES[name]).cuda(), return_gradients=True)
    assert e.dtype == torch.bool and e.is_cuda and g.is_cuda
    assert tuple(e.shape) == CASES[name].shape[:3] and tuple(g.shape) == (e.shape[0], 3) + tuple(e.shape[1:])
    return e.cpu().numpy(), g.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gradients_match_float64(name):
    _, g = _device(name)
    for k in range(len(CASES[name])):
        g64 = _ref64(name)[k][1]
        err = [float(np.abs(g64[c] - g[k, c]).max()) for c in range(3)]
        print(f"{name}[{k}]: max |gi, gj, m - float64| = {err[0]:.3e}, {err[1]:.3e}, {err[2]:.3e}")
        assert max(err) <= GRAD_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_decisions_are_exact_on_the_device_gradients(name):
    e, g = _device(name)
    for k in range(len(CASES[name])):
        assert g[k].dtype == np.float32
        want = R.decide(g[k, 0], g[k, 1], g[k, 2], 0.1, 0.2)
        assert (e[k] == want).all(), int((e[k] != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_against_float64(name):
    e, g = _device(name)
    for k in range(len(CASES[name])):
        _end_to_end(name, k, e[k], g[k])


def _hysteresis_device(cls):
    return execute(BUILDERS["camo_canny_hysteresis"](cls), 0xFF)["edges"]


def _serpentine(n=128):
    """A one-pixel-wide path of weak pixels through every even row, joined alternately at the right and the left end."""
    cls = np.zeros((1, n, n), np.uint8)
    cls[0, 0::2] = 1
    for r in range(1, n - 1, 2):
        cls[0, r, n - 1 if r % 4 == 1 else 0] = 1
    return cls


@pytest.mark.gpu
def test_hysteresis_follows_a_serpentine_through_every_tile():
    cls = _serpentine()
    from scipy import ndimage
    assert ndimage.label(cls[0] > 0, structure=R.ALL8)[1] == 1 and cls[0, 126, 0] == 1 and cls[0, 0, 0] == 1
    assert not _hysteresis_device(cls).any()                                  # no strong pixel: nothing kept
    cls[0, 126, 0] = 2                                                        # the far end of the path that starts at (0, 0)
    out = _hysteresis_device(cls)
    assert set(np.unique(out)) <= {0, 1} and ((out > 0) == (cls > 0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seed", [((2, 70, 33), 0), ((1, 128, 128), 1)])
def test_hysteresis_on_random_class_maps(shape, seed):
    rs = np.random.RandomState(seed)
    u = rs.uniform(0, 1, shape)
    cls = (u < 0.42).astype(np.uint8) + (u < 0.004)                           # weak near the 8-connected percolation threshold, few strong
    want = np.stack([R.hysteresis(c) for c in cls])
    assert 0 < want.sum() < (cls > 0).sum()
    a, b = _hysteresis_device(cls), _hysteresis_device(cls)
    assert ((a > 0) == want).all(), int(((a > 0) != want).sum())
    assert a.tobytes() == b.tobytes()


def _solid_class_maps():
    """Class maps of solid weak regions -- what the run parents and the left-out unions of csrc/cc_inl.h are for; the maps
    above are sparse."""
    from test_instances import _ring
    full = np.ones((1, 70, 33), np.uint8)
    one_strong = full.copy()
    one_strong[0, -1, -1] = 2                                                 # the last index: the root is the first
    squares = np.zeros((1, 64, 64), np.uint8)                                 # they touch diagonally only, at a tile corner
    squares[0, 12:32, 12:32] = 1
    squares[0, 32:52, 32:52] = 1
    squares[0, 40, 45] = 2
    u = np.random.RandomState(5).uniform(0, 1, (2, 70, 33))
    dense = (u < 0.9).astype(np.uint8) + (u < 0.001)
    m = np.zeros((45, 70), bool)                                              # a wall without its corner: its ends meet diagonally
    _ring(m, 10, 10, 40, 50)
    m[10, 10] = False
    ring = m.astype(np.uint8)[None]
    ring[0, 10, 11] = 2
    return {"all weak, one strong": one_strong, "all weak": full, "corner squares": squares, "dense": dense, "ring with a gap": ring}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all weak, one strong", "all weak", "corner squares", "dense", "ring with a gap"])
def test_hysteresis_on_solid_class_maps(name):
    cls = _solid_class_maps()[name]
    want = np.stack([R.hysteresis(c) for c in cls])
    a, b = _hysteresis_device(cls), _hysteresis_device(cls)
    assert ((a > 0) == want).all(), int(((a > 0) != want).sum())
    assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_batch_equals_singles():
    import torch
    from camouflage_multimodal_amd import canny_edges
    e, g = _device("3x96x80")
    for k, im in enumerate(CASES["3x96x80"]):
        e1, g1 = canny_edges(torch.from_numpy(im).cuda(), return_gradients=True)
        assert tuple(e1.shape) == (96, 80) and tuple(g1.shape) == (3, 96, 80)
        assert e1.cpu().numpy().tobytes() == e[k].tobytes() and g1.cpu().numpy().tobytes() == g[k].tobytes()


@pytest.mark.gpu
def test_region_graph_computes_its_own_edge_map():
    import torch
    from camouflage_multimodal_amd import canny_edges, create_region_graph_from_segments
    from oracle import rg_features_oracle as RO
    img = CASES["3x96x80"][0]
    seg = RO.voronoi_segments(96, 80, 30, 2)
    edges = canny_edges(img)
    assert edges.dtype == torch.bool and edges.is_cuda and edges.any()
    d0, r0 = create_region_graph_from_segments(img, seg)
    d1, r1 = create_region_graph_from_segments(img, seg, edges)
    for a, b in ((d0.x, d1.x), (d0.edge_index, d1.edge_index), (d0.edge_attr, d1.edge_attr), (r0, r1)):
        assert a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    x, ei, ea, rmap = RO.region_graph(img, seg, edges.cpu().numpy())
    assert x[:, 13].max() > 0                                                 # the edge-density feature sees the map
    assert (r0.cpu().numpy() == rmap).all()
    gx = d0.x.cpu().numpy()
    scale = np.maximum(np.abs(x).max(0), 1e-3)
    assert gx.shape == x.shape and (np.abs(gx - x) <= 2e-6 * scale + 2e-6 * np.abs(x)).all()
    assert (d0.edge_index.cpu().numpy() == ei).all()
    ga = d0.edge_attr.cpu().numpy()
    assert ga.shape == (ea.shape[0], 1) and (np.abs(ga[:, 0] - ea) <= 2e-5 * ea + 1e-9).all()
