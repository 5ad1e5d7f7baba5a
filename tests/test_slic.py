"""SLIC label maps on the device (include/camo_slic.h) against tests/slic_ref.py.

PARITY UNPINNED (skimage absent): the header's text is the definition and the checker restates it with numpy / scipy.ndimage.
CPU tests hold the checker to scipy's Gaussian filter, to textbook Lab values and to hand cases of the connectivity step, and
show that the three small cases are decided with clear margins, so that float32 arithmetic cannot change a label.  GPU tests
hold the HIP kernels to the checker, stage by stage and end to end:

  preprocess    |lab - float64| <= 4 x the float32 restatement's own largest error on the same case (device powf / cbrtf may
                be a few ulp looser than numpy's)
  assign        nearest and dist equal the float32 restatement bit for bit, on the float64 trajectory cast to fp32
  update        equal to the float32 restatement bit for bit; against float64 means: colours 2^-25 + 2^-24 |m| (the 2^-24
                fixed point of the sums rounds each pixel by at most 2^-25, the fp32 result by half an ulp), coordinates 2^-24 |m|;
                bit for bit also on maps with more labels in a tile than the tile's table has slots
  connect       equal to the sequential loop, exactly
  end to end    the three clear-margin cases equal the float64 reference exactly

TAU = 2.1e-4 is 8 x the largest |dist - float64| (2.584e-5, at 96 x 80 image 0, iteration 0, where the zero initial colour makes
d about 100), rounded up.  That figure is the float32 restatement's, which the device must equal bit for bit, so it is
checked on the CPU too.  Smallest float64 margins of the clear-margin cases: 20 x 28 5.90e-3 and 8.20e-4, 33 x 70
1.36e-3 and 1.72e-3, 96 x 80 2.38e-4 and 2.40e-4.  Measured on an MI355X: preprocess error at most 6.6e-6 (the float32
restatement's own: 6.2e-6 to 9.7e-6), |dist - float64| as above, update error at most 0.96 of its bound; DESIGN.md 10b
records the figures.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import slic_ref as R
from conftest import ROOT
from raw_calls import BUILDERS, execute

TAU = 2.1e-4
CASES = R.cases()
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def _ref(name, k, f32=False):
    """(lab, records of the ten iterations) of image k of a case in float64 (or float32).  Computed once, never written to."""
    H, W, n, _ = R.TABLE[name]
    dt = np.float32 if f32 else np.float64
    lab = R.preprocess(CASES[name][0][k], dtype=dt)
    return lab, R.iterate(lab, R.grid(H, W, n), dt)


@functools.lru_cache(maxsize=None)
def _ref_labels(name, k, f32=False):
    H, W, n, _ = R.TABLE[name]
    g = R.grid(H, W, n)
    return R.connect(_ref(name, k, f32)[1][-1]["near"] + 1, *R.sizes(H, W, g["K"]))


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_grid_table_and_refusals():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int32 * 5)()
    for name, (H, W, n, (step, start, ny, nx, K)) in R.TABLE.items():
        assert R.grid(H, W, n) == dict(K=K, step=step, start=start, ny=ny, nx=nx), name
        assert L.camo_slic_grid(H, W, n, out) == 0 and tuple(out) == (K, step, start, ny, nx), (name, tuple(out))
    for H, W, n in ((4, 5, 20), (4, 5, 21), (3, 400, 2)):                  # n_segments >= H W (twice), min(H, W) < s
        with pytest.raises(ValueError):
            R.grid(H, W, n)
        assert L.camo_slic_grid(H, W, n, out) == -2, (H, W, n)
    assert L.camo_slic_grid(256, 256, 0, out) == -1 and L.camo_slic_grid(256, 256, 500, None) == -1
    assert L.camo_slic_grid(256, 256, 5000, out) == -2 and b"MAX_LABELS" in L.camo_last_error()
    c = R.initial_centroids(R.grid(20, 28, 12))
    assert c.shape == (12, 5) and tuple(c[5]) == (10, 10, 0, 0, 0) and tuple(c[11]) == (17, 24, 0, 0, 0)


def test_smoothing_equals_scipy_and_lab_textbook_values():
    from scipy import ndimage
    for name in NAMES[:3]:
        v = R.quantise(CASES[name][0][0])
        assert v.min() >= 0 and v.max() <= 1 and np.abs(v * 255 - np.rint(v * 255)).max() < 1e-12
        for sigma in (1.0, 2.0):
            got = R.smooth(v, sigma)
            for c in range(3):
                assert np.abs(got[..., c] - ndimage.gaussian_filter(v[..., c], sigma, mode="reflect")).max() <= 1e-12
        assert (R.smooth(v, 0.0) == v).all()
    assert len(R.gaussian_weights(1.0)) == 9 and abs(R.gaussian_weights(1.0).sum() - 1) < 1e-15
    for rgb, want in (((0, 0, 0), (0, 0, 0)), ((1, 1, 1), (100, 0, 0)), ((1, 0, 0), (53.24, 80.09, 67.20))):
        for dt in (np.float64, np.float32):
            got = R.lab_scaled(np.array(rgb, np.float64), 1.0, dt)
            assert got.dtype == dt and np.abs(got - np.array(want)).max() <= 0.01, (rgb, got)
    assert np.abs(R.lab_scaled(np.array([1.0, 0, 0]), 10.0) * 10 - R.lab_scaled(np.array([1.0, 0, 0]), 1.0)).max() < 1e-12
    assert R.quantise(np.array([0.999, 1.0, 1.5, -0.2], np.float32)).tolist() == [254 / 255, 1.0, 1.0, 0.0]


def test_binding_and_argument_checks_without_a_gpu():
    from camouflage_multimodal_amd import _lib, slic_segments, region_graph_from_image, predict_from_image  # noqa: F401
    hdr = open(os.path.join(ROOT, "include", "camo_slic.h")).read()
    assert "PARITY UNPINNED" in hdr
    L = _lib.lib()
    assert L.camo_abi_version() == 13
    need = L.camo_slic_workspace_bytes(2, 96, 80, 60)
    conn = L.camo_slic_workspace_bytes(2, 96, 80, 0)
    assert conn >= 2 * 96 * 80 * 17 and need >= conn + 2 * 96 * 80 * 16 + 2 * 63 * (20 + 48)
    assert L.camo_slic_workspace_bytes(0, 96, 80, 60) == 0 and b"N >= 1" in L.camo_last_error()
    assert L.camo_slic_workspace_bytes(1, 96, 0, 60) == 0
    assert L.camo_slic_workspace_bytes(1, 4, 5, 20) == 0 and b"n_segments" in L.camo_last_error()
    assert L.camo_slic_workspace_bytes(64, 8192, 8192, 500) == 0 and b"PIXELS" in L.camo_last_error()
    p = ctypes.c_void_p(0x1000)                                              # (never dereferenced: every check comes before any launch)

    def call(N=1, H=96, W=80, n=60, compactness=10.0, sigma=1.0, img=p, ws=p, nbytes=None, labels=p, counts=p):
        return L.camo_slic(img, N, H, W, n, compactness, sigma, ws, L.camo_slic_workspace_bytes(1, 96, 80, 60) if nbytes is None else nbytes,
                           labels, counts, None)
    assert call(N=0) == -1 and call(H=0) == -1 and call(W=-3) == -1 and call(n=0) == -1
    assert call(n=96 * 80) == -2 and call(H=3, W=400, n=2) == -2
    assert call(compactness=0.0) == -1 and call(compactness=float("nan")) == -1 and call(compactness=0.01) == -2 and b"compactness" in L.camo_last_error()
    assert call(sigma=-1.0) == -1 and b"sigma" in L.camo_last_error()
    assert call(sigma=9.0) == -2 and b"radius" in L.camo_last_error()
    assert call(img=None) == -1 and call(ws=None) == -1 and call(labels=None) == -1 and call(counts=None) == -1 and b"null" in L.camo_last_error()
    assert call(nbytes=L.camo_slic_workspace_bytes(1, 96, 80, 60) - 1) == -3 and b"camo_slic_workspace_bytes" in L.camo_last_error()
    assert L.camo_slic_preprocess(None, 1, 8, 8, 10.0, 1.0, p, None) == -1 and L.camo_slic_preprocess(p, 1, 8, 8, 10.0, 9.0, p, None) == -2
    assert L.camo_slic_assign(p, p, 1, 8, 8, 0, 3, p, p, None) == -1 and L.camo_slic_assign(p, p, 1, 8, 8, 4, 0, p, p, None) == -1
    assert L.camo_slic_assign(p, None, 1, 8, 8, 4, 3, p, p, None) == -1 and L.camo_slic_assign(p, p, 1, 8, 8, 4096, 3, p, p, None) == -1
    assert L.camo_slic_update(p, p, 1, 8, 8, 4, None, p, None) == -1 and L.camo_slic_update(p, p, 1, 8, 0, 4, p, p, None) == -1
    assert L.camo_slic_connect(None, 1, 8, 8, 2, 10, p, 1 << 20, p, p, None) == -1
    assert L.camo_slic_connect(p, 1, 8, 8, -1, 10, p, 1 << 20, p, p, None) == -1 and L.camo_slic_connect(p, 1, 8, 8, 2, 0, p, 1 << 20, p, p, None) == -1
    assert L.camo_slic_connect(p, 1, 8, 8, 2, 10, p, 16, p, p, None) == -3
    import torch
    with pytest.raises(_lib.CamoError):
        slic_segments(torch.zeros(16, 16, 3), 4)
    with pytest.raises(_lib.CamoError):
        region_graph_from_image(np.zeros((16, 16, 3), np.float32), 4, device="cpu")


def _hand_maps():
    """name -> (label map, min_size, expected output)."""
    island = np.full((12, 12), 5, np.int32); island[4:6, 7:9] = 7
    first = np.full((6, 8), 4, np.int32); first[0, :2] = 3
    want_first = np.ones((6, 8), np.int32); want_first[0, :2] = 0
    chain = np.full((6, 10), 1, np.int32); chain[:, 6:] = 9; chain[0, 6:] = (2, 3, 4, 5)
    want_chain = np.ones((6, 10), np.int32); want_chain[1:, 6:] = 2
    return {"island": (island, 10, np.ones((12, 12), np.int32)), "first": (first, 5, want_first), "chain": (chain, 5, want_chain)}


def test_connectivity_hand_cases():
    for name, (seg, min_size, want) in _hand_maps().items():
        out, over = R.connect(seg, min_size, 10 ** 6)
        assert (out == want).all() and over == 0, (name, out)
        assert (R.connect(seg, min_size, 10 ** 6, cut=True)[0] == want).all()
        assert R.four_connected(out, ignore=(0,))
    # a single-pixel neighbour order case: the last foreign labelled neighbour in the order +x, -x, +y, -y stands
    seg = np.array([[1, 1, 1, 2, 2, 2], [1, 1, 1, 2, 2, 2], [1, 1, 7, 2, 2, 2]], np.int32)       # (2, 2): -x is label 1, +x is label 2, -y is label 1
    out, _ = R.connect(seg, 3, 100)
    assert out[2, 2] == 1 and out[0, 0] == 1 and out[0, 3] == 2
    # the cut splits a component of max_size pixels or more; without it the component stays whole and is counted
    big = np.zeros((4, 10), np.int32)
    whole, over = R.connect(big, 2, 16)
    parts, _ = R.connect(big, 2, 16, cut=True)
    assert over == 1 and (whole == 1).all() and len(np.unique(parts)) > 1


@pytest.mark.parametrize("name", R.CLEAR)
def test_small_cases_are_decided_with_clear_margins(name):
    H, W, n, _ = R.TABLE[name]
    step = R.grid(H, W, n)["step"]
    for k in range(len(CASES[name][0])):
        lab64, rec = _ref(name, k)
        smallest, worst = np.inf, 0.0
        for it, r in enumerate(rec):
            m = r["second"] - r["best"]
            tie = m == 0
            assert not tie.any() or (it == 0 and step % 2 == 0), (name, k, it)
            smallest = min(smallest, float(m[~tie].min()))
            assert not r["soft"].any(), (name, k, it)
            if it in (0, 1, 9):
                _, b32, _, _ = R.assign(lab64.astype(np.float32), r["cent"].astype(np.float32), step, np.float32)
                worst = max(worst, float(np.abs(b32.astype(np.float64) - r["best"]).max()))
        print(f"{name}[{k}]: smallest float64 margin {smallest:.3e}, float32 restatement max |dist - float64| {worst:.3e}")
        assert smallest >= TAU and 8 * worst <= TAU
        rec32 = _ref(name, k, True)[1]
        assert all((a["near"] == b["near"]).all() for a, b in zip(rec, rec32))
        assert (_ref_labels(name, k)[0] == _ref_labels(name, k, True)[0]).all()
    if step % 2 == 0:
        assert (rec[0]["second"] == rec[0]["best"]).any()                    # 33 x 70: the lowest-k tie rule is exercised


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(fn, *args):
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    import torch
    L = _lib.lib()
    _lib.check(getattr(L, fn)(*[_ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _stream_ptr()), fn)


def _preprocess_device(images, compactness=10.0, sigma=1.0):
    import torch
    img = _cuda(images)
    N, H, W = img.shape[:3]
    lab = torch.empty(N, H, W, 3, dtype=torch.float32, device="cuda")
    _call("camo_slic_preprocess", img, N, H, W, compactness, sigma, lab)
    return lab


def _assign_device(lab, cent, step):
    import torch
    N, H, W = lab.shape[:3]
    near = torch.empty(N, H, W, dtype=torch.int32, device="cuda")
    dist = torch.empty(N, H, W, dtype=torch.float32, device="cuda")
    _call("camo_slic_assign", lab, cent, N, H, W, cent.shape[1], step, near, dist)
    return near, dist


def _update_device(lab, near, cent):
    """camo_slic_update on guarded buffers, numpy in and out; ``sums`` starts from 0x7F bytes (scratch: any content)."""
    return execute(BUILDERS["camo_slic_update"](lab, near, cent), 0x7F)["centroids"]


def _connect_device(maps, min_size, max_size):
    got = execute(BUILDERS["camo_slic_connect"](np.asarray(maps, np.int32), min_size, max_size), 0xFF)
    return got["labels"], got["counts"]


@functools.lru_cache(maxsize=None)
def _device(name):
    """(labels int32 [N, H, W], counts [N, 2]) of a case's batch as numpy; one call per case for all tests."""
    import torch
    from camouflage_multimodal_amd import slic_segments
    images, n = CASES[name]
    lab, cnt = slic_segments(_cuda(images), n, return_counts=True)
    assert lab.dtype == torch.int32 and lab.is_cuda and tuple(lab.shape) == images.shape[:3] and tuple(cnt.shape) == (len(images), 2)
    return lab.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_preprocess_matches_float64(name):
    images = CASES[name][0]
    got = _preprocess_device(images).cpu().numpy()
    for k in range(len(images)):
        lab64 = _ref(name, k)[0]
        own = float(np.abs(R.preprocess(images[k], dtype=np.float32).astype(np.float64) - lab64).max())
        err = float(np.abs(got[k].astype(np.float64) - lab64).max())
        print(f"{name}[{k}]: max |lab - float64| = {err:.3e}, float32 restatement {own:.3e}")
        assert err <= 4 * own
    for sigma in (0.0, 2.0):
        g = _preprocess_device(images[:1], sigma=sigma).cpu().numpy()[0].astype(np.float64)
        r64 = R.preprocess(images[0], sigma=sigma)
        own = float(np.abs(R.preprocess(images[0], sigma=sigma, dtype=np.float32).astype(np.float64) - r64).max())
        assert np.abs(g - r64).max() <= 4 * own


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_assign_equals_the_float32_restatement_bit_for_bit(name):
    H, W, n, _ = R.TABLE[name]
    step = R.grid(H, W, n)["step"]
    N = len(CASES[name][0])
    worst = 0.0
    for it in (0, 1, 9):
        lab = np.stack([_ref(name, k)[0] for k in range(N)]).astype(np.float32)
        cent = np.stack([_ref(name, k)[1][it]["cent"] for k in range(N)]).astype(np.float32)
        near, dist = (t.cpu().numpy() for t in _assign_device(_cuda(lab), _cuda(cent), step))
        for k in range(N):
            n32, b32, _, _ = R.assign(lab[k], cent[k], step, np.float32)
            assert (near[k] == n32).all(), (it, k, int((near[k] != n32).sum()))
            assert dist[k].tobytes() == b32.tobytes(), (it, k)
            worst = max(worst, float(np.abs(dist[k].astype(np.float64) - _ref(name, k)[1][it]["best"]).max()))
    print(f"{name}: max |dist - float64| = {worst:.3e}")
    if name in R.CLEAR:
        assert 8 * worst <= TAU


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_update_against_float64_means(name):
    N = len(CASES[name][0])
    lab = np.stack([_ref(name, k)[0] for k in range(N)]).astype(np.float32)
    near = np.stack([_ref(name, k)[1][4]["near"] for k in range(N)])
    cent = np.stack([_ref(name, k)[1][4]["cent"] for k in range(N)]).astype(np.float32)
    K = cent.shape[1]
    near = near.copy()
    near[near == 1] = 0; near[near == K - 2] = K - 1                          # two centroids left without a pixel
    a, b = _update_device(lab, near, cent), _update_device(lab, near, cent)
    assert a.tobytes() == b.tobytes()
    for k in range(N):
        assert a[k, 1].tobytes() == cent[k, 1].tobytes() and a[k, K - 2].tobytes() == cent[k, K - 2].tobytes()
        want = R.update(lab[k].astype(np.float64), near[k], cent[k].astype(np.float64), np.float64)
        err = np.abs(a[k].astype(np.float64) - want)
        bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -40
        bound[:, 2:] += 2.0 ** -25
        print(f"{name}[{k}]: max update error / bound = {float((err / bound).max()):.3f}, max error {float(err.max()):.3e}")
        assert (err <= bound).all()
        assert a[k].tobytes() == R.update(lab[k], near[k], cent[k], np.float32).tobytes()


def _tile_labels(near):
    """Distinct labels in each 32 x 32 tile of one map, tiles in reading order."""
    H, W = near.shape
    return [len(np.unique(near[y:y + 32, x:x + 32])) for y in range(0, H, 32) for x in range(0, W, 32)]


# A tile's table holds 128 labels; real assignments stay far below that, so these maps are made to pass it: name -> (side, K,
# near of the side x side pixels, distinct labels per tile).  Every pixel its own centroid; the same over four tiles; and every
# centroid collecting pixels from several tiles, some through a table and some past a full one.
FULL_TABLE_MAPS = {
    "32x32 arange": (32, 1024, lambda n: np.arange(n), [1024]),
    "40x40 arange": (40, 1600, lambda n: np.arange(n), [1024, 256, 256, 64]),
    "40x40 stride 7 mod 300": (40, 300, lambda n: np.arange(n) * 7 % 300, [300, 120, 244, 64]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FULL_TABLE_MAPS))
def test_update_past_a_full_tile_table_bit_for_bit(name):
    side, K, fill, per_tile = FULL_TABLE_MAPS[name]
    near = fill(side * side).reshape(side, side).astype(np.int32)
    assert _tile_labels(near) == per_tile and max(per_tile) > 128
    rs = np.random.RandomState(side + K)
    lab = rs.uniform(-1.0, 1.0, (side, side, 3)).astype(np.float32)
    cent = rs.uniform(0.0, side, (K, 5)).astype(np.float32)
    want = R.update(lab, near, cent, np.float32)
    a, b = _update_device(lab[None], near[None], cent[None]), _update_device(lab[None], near[None], cent[None])
    assert a.tobytes() == b.tobytes()
    assert a[0].tobytes() == want.tobytes(), int((a[0] != want).sum())


def _check_connect(maps, min_size, max_size, oversized=False):
    maps = np.asarray(maps, np.int32)
    got, counts = _connect_device(maps, min_size, max_size)
    again, counts2 = _connect_device(maps, min_size, max_size)
    assert got.tobytes() == again.tobytes() and counts.tobytes() == counts2.tobytes()
    for k, seg in enumerate(maps):
        want, over = R.connect(seg, min_size, max_size)
        assert (got[k] == want).all(), (k, int((got[k] != want).sum()))
        assert counts[k, 0] == want.max() + 1 and counts[k, 1] == over
        if oversized:
            assert over >= 1
        else:
            assert over == 0 and (R.connect(seg, min_size, max_size, cut=True)[0] == want).all()
            assert R.four_connected(want, ignore=(0,))
    return got


@pytest.mark.gpu
def test_connect_hand_cases_and_checkerboard():
    for name, (seg, min_size, want) in _hand_maps().items():
        assert (_check_connect(seg[None], min_size, 10 ** 6)[0] == want).all(), name
    yy, xx = np.meshgrid(np.arange(40), np.arange(70), indexing="ij")
    board = ((yy + xx) % 2).astype(np.int32)
    assert (_check_connect(board[None], 3, 10 ** 6) == 0).all()               # every pixel a small component: chains of adoptions to none
    assert (_check_connect(board[None], 1, 10 ** 6)[0] == 1 + np.arange(2800).reshape(40, 70)).all()
    assert (_check_connect(board[None], 0, 10 ** 6)[0] == 1 + np.arange(2800).reshape(40, 70)).all()


@pytest.mark.gpu
def test_connect_follows_a_serpentine_through_every_tile():
    n = 128
    seg = np.zeros((1, n, n), np.int32)
    seg[0, 0::2] = 1
    for r in range(1, n - 1, 2):
        seg[0, r, n - 1 if r % 4 == 1 else 0] = 1
    got = _check_connect(seg, 200, 10 ** 6)                                   # the path is one large component; the 127-pixel strips adopt
    assert set(np.unique(got)) == {1}
    got = _check_connect(seg, 100, 10 ** 6)                                   # the strips are large too
    assert got.max() == 65                                                    # the path, 63 strips of 127 pixels and the last row


@pytest.mark.gpu
@pytest.mark.parametrize("shape,seed", [((2, 70, 33), 0), ((1, 128, 128), 1)])
def test_connect_on_salted_voronoi_maps(shape, seed):
    from oracle import rg_features_oracle as RO
    rs = np.random.RandomState(seed)
    N, H, W = shape
    maps = np.stack([RO.voronoi_segments(H, W, 30, seed + 7 * i) for i in range(N)]).astype(np.int32)
    salt = rs.uniform(0, 1, shape) < 0.02
    maps[salt] = rs.randint(0, 30, int(salt.sum()))
    got = _check_connect(maps, 6, 10 ** 6)
    assert got.max() >= 10
    big = _check_connect(maps, 6, 60, oversized=True)                         # the same maps with a small max_size: left whole, and counted
    assert (big == got).all()


def _solid_label_maps():
    """Label maps of large equal-label regions -- what the run parents and the left-out unions of csrc/cc_inl.h are for; the maps
    above are thin paths and Voronoi cells."""
    squares = np.zeros((1, 64, 64), np.int32)                                 # label 1 touches itself diagonally only, at a tile corner:
    squares[0, 12:32, 12:32] = 1                                              # two components at 4-connectivity
    squares[0, 32:52, 32:52] = 1
    xx = np.broadcast_to(np.arange(70), (1, 70, 70))
    maps = {"corner squares": squares, "one label": np.full((1, 33, 33), 7, np.int32),
            "random": np.random.RandomState(11).randint(0, 3, (2, 70, 33)).astype(np.int32)}
    for w in (1, 2, 33):
        maps[f"stripes of {w}"] = (xx // w % 2).astype(np.int32)
    return maps


@pytest.mark.gpu
@pytest.mark.parametrize("min_size", [0, 5])
@pytest.mark.parametrize("name", ["corner squares", "stripes of 1", "stripes of 2", "stripes of 33", "one label", "random"])
def test_connect_on_solid_label_maps(name, min_size):
    got = _check_connect(_solid_label_maps()[name], min_size, 10 ** 6)
    if name == "corner squares":
        assert got[0, 12, 12] != got[0, 32, 32] and got.max() == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_whole_call_equals_its_stages_and_a_batch_its_images(name):
    import torch
    from camouflage_multimodal_amd import slic_segments
    images, n = CASES[name]
    N, H, W = images.shape[:3]
    g = R.grid(H, W, n)
    labels, counts = _device(name)
    lab = _preprocess_device(images)
    lab_host = lab.cpu().numpy()
    cent = np.stack([R.initial_centroids(g, np.float32)] * N)
    for it in range(R.ITERATIONS):
        near = _assign_device(lab, _cuda(cent), g["step"])[0].cpu().numpy()
        cent = _update_device(lab_host, near, cent)
    got, cnt = _connect_device(near, *R.sizes(H, W, g["K"]))
    assert got.tobytes() == labels.tobytes() and cnt.tobytes() == counts.tobytes()
    again, counts2 = slic_segments(_cuda(images), n, return_counts=True)
    assert again.cpu().numpy().tobytes() == labels.tobytes() and counts2.cpu().numpy().tobytes() == counts.tobytes()
    for k in range(N):
        one, c1 = slic_segments(torch.from_numpy(images[k]).cuda(), n, return_counts=True)
        assert tuple(one.shape) == (H, W) and one.cpu().numpy().tobytes() == labels[k].tobytes() and c1.cpu().numpy().tobytes() == counts[k].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.CLEAR)
def test_end_to_end_equals_float64(name):
    labels, counts = _device(name)
    for k in range(len(labels)):
        want, over = _ref_labels(name, k)
        assert (labels[k] == want).all(), (k, int((labels[k] != want).sum()))
        assert counts[k, 0] == want.max() + 1 and counts[k, 1] == over


@pytest.mark.gpu
def test_256_sanity():
    labels, counts = _device("256x256")
    K = R.TABLE["256x256"][3][4]
    for k in range(len(labels)):
        print(f"256x256[{k}]: {counts[k, 0] - 1} labels of K = {K}, oversized components {counts[k, 1]}")
        assert 0.5 * K <= counts[k, 0] - 1 <= K and labels[k].max() == counts[k, 0] - 1 and labels[k].min() >= 0
        if counts[k, 1] == 0:
            assert R.four_connected(labels[k], ignore=(0,))


@pytest.mark.gpu
def test_region_graph_and_prediction_from_the_image(kg_real):
    import torch
    from camouflage_multimodal_amd import (RegionGraphGNN, build_multimodal_model, create_region_graph_from_segments, predict_from_image,
                                           predict_from_region_graph, region_graph_from_image, slic_segments)
    # the noise image: camo_rg_region_graph takes a region's colour variance as a difference of float64 sums that it adds with
    # atomics, so on a region of one flat colour (the blob images saturate to such regions) that variance is rounding noise
    # of the order the additions arrived in, and two calls on the SAME segments need not agree in its last bits
    img = CASES["96x80"][0][1]
    data, seg = region_graph_from_image(img, 60)
    assert seg.is_cuda and seg.dtype == torch.int32 and seg.cpu().numpy().tobytes() == _device("96x80")[0][1].tobytes()
    d2, _ = create_region_graph_from_segments(img, slic_segments(img, 60))
    for a, b in ((data.x, d2.x), (data.edge_index, d2.edge_index), (data.edge_attr, d2.edge_attr)):
        assert a.is_cuda and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert data.x.shape[0] >= 30 and data.edge_index.shape[1] > 0
    torch.manual_seed(1)
    rgm = RegionGraphGNN().cuda().eval()
    fm = build_multimodal_model({}).cuda().eval().set_precision("f32")
    kg = {f"cat{i:02d}": torch.from_numpy(kg_real[i:i + 1]) for i in range(13)}
    p1, attn, _ = predict_from_image(fm, rgm, img, kg, "cuda", n_segments=60)
    p2, _, _ = predict_from_region_graph(fm, rgm, data, kg, "cuda")
    # (equal up to the summation order of the fusion model's atomically accumulated mean pools, as in test_rg_gnn.py)
    assert torch.allclose(p1["mask_logits"], p2["mask_logits"], rtol=0, atol=1e-6) and p1["mask_pred"] == p2["mask_pred"]
    assert abs(p1["score"] - p2["score"]) < 1e-6 and attn is not None
