"""Edge-aware mask refinement (include/camo_guided.h) against tests/guided_ref.py.

PARITY UNPINNED: the header is the definition and the float64 numpy restatement (every window summed directly) the checker.  CPU tests
hold the restatement to a plain Python double loop and to the properties a guided filter has by construction, the host argument
checks to the header, and the definition itself to what it is for: the IoU it gains on the disc case.  GPU tests hold the kernels
to the restatement per pixel within

    q      4 * 2^-24 * (sum_c |abar_c I_c| + |bbar| + 1)
    coef   4 * 2^-24 * (|abar_c| + 1)   and   4 * 2^-24 * (|bbar| + |abar . mu| + 1)
    apply  2^-23 * |ref| + 2^-45 * sum |terms|

with every magnitude taken from the restatement's own values.  The bound is derived, not tuned: a model that accumulates in double
and rounds a, b, abar, bbar and q to fp32 once each stays at <= 0.76 of 2^-24 (...) against the float64 reference; the factor 4
is the margin for another summation order and FMA contraction.  Every test prints its measured maximum as a fraction of the bound.

The shapes are the smallest at which the kernels can go wrong: one pixel, one row, one column, windows larger than the image
(r = 8 on 5 x 7, r = 64 on 45 x 70), sizes that are no multiple of the 256-thread block and more than one block.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import guided_ref as R
import resize_ref as RR
from conftest import ROOT

E_ARG = -1
# (shape, radius, C, eps, guide kind, p kind, N): every shape, radius, C, eps, kind and N of the issue's list appears
FILTER_CASES = (
    ((1, 1), 1, 1, 1e-2, "uniform", "uniform", 1),
    ((1, 70), 3, 3, 1e-4, "binary", "binary", 1),
    ((70, 1), 8, 1, 1e-6, "near", "uniform", 1),
    ((5, 7), 8, 3, 1e-4, "uniform", "binary", 5),
    ((5, 7), 64, 1, 1e-2, "binary", "uniform", 1),
    ((33, 33), 32, 3, 1e-6, "near", "binary", 1),
    ((33, 33), 3, 1, 1e-4, "uniform", "uniform", 5),
    ((45, 70), 8, 3, 1e-6, "binary", "uniform", 1),
    ((45, 70), 64, 3, 1e-4, "uniform", "binary", 1),
    ((64, 96), 8, 3, 1e-4, "uniform", "uniform", 1),
    ((64, 96), 32, 1, 1e-6, "binary", "binary", 1),
    ((64, 96), 1, 3, 1e-2, "near", "uniform", 1),
)


@functools.lru_cache(maxsize=None)
def _filter_case(i):
    """(guide fp32 [N, H, W, C], p fp32 [N, H, W], the reference dicts per image); never written to."""
    (H, W), r, C, eps, gk, pk, N = FILTER_CASES[i]
    guide = np.stack([R.make_guide(gk, H, W, C, 100 * i + n) for n in range(N)])
    p = np.stack([R.make_p(pk, H, W, 100 * i + n) for n in range(N)])
    return guide, p, [R.guided_filter(guide[n], p[n], r, eps) for n in range(N)]


@functools.lru_cache(maxsize=None)
def _disc(guide, r, eps):
    img, p, disc = R.disc_case()
    return R.guided_filter(img if guide == "rgb" else R.grey(img), p, r, eps)


# ---- CPU: the restatement --------------------------------------------------------------------------------------------------------------
def _loop_filter(I, p, r, eps):
    """The header in plain Python floats (doubles), pixel by pixel."""
    H, W, C = I.shape
    I, p = I.astype(float).tolist(), p.astype(float).tolist()

    def window(y, x):
        return [(yy, xx) for yy in range(max(y - r, 0), min(y + r, H - 1) + 1) for xx in range(max(x - r, 0), min(x + r, W - 1) + 1)]
    a = [[None] * W for _ in range(H)]
    b = [[None] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            w = window(y, x)
            n = float(len(w))
            mu = [sum(I[yy][xx][c] for yy, xx in w) / n for c in range(C)]
            pbar = sum(p[yy][xx] for yy, xx in w) / n
            cov = [sum(I[yy][xx][c] * p[yy][xx] for yy, xx in w) / n - mu[c] * pbar for c in range(C)]
            S = [[sum(I[yy][xx][i] * I[yy][xx][j] for yy, xx in w) / n - mu[i] * mu[j] + (eps if i == j else 0.0) for j in range(C)] for i in range(C)]
            av = np.linalg.solve(np.array(S), np.array(cov)).tolist()
            a[y][x], b[y][x] = av, pbar - sum(av[c] * mu[c] for c in range(C))
    q = np.empty((H, W))
    for y in range(H):
        for x in range(W):
            w = window(y, x)
            n = float(len(w))
            abar = [sum(a[yy][xx][c] for yy, xx in w) / n for c in range(C)]
            q[y, x] = sum(abar[c] * I[y][x][c] for c in range(C)) + sum(b[yy][xx] for yy, xx in w) / n
    return q


@pytest.mark.parametrize("r", (1, 8))
@pytest.mark.parametrize("C", (1, 3))
def test_reference_is_the_double_loop(r, C):
    I, p = R.make_guide("uniform", 5, 7, C, 7 + C), R.make_p("uniform", 5, 7, 9)
    ref = R.guided_filter(I, p, r, 1e-3)
    assert np.abs(ref["q"] - _loop_filter(I, p, r, 1e-3)).max() < 1e-12


def test_reference_properties():
    one = R.guided_filter(np.float32([[[0.3, 0.6, 0.9]]]), np.float32([[0.7]]), 8, 1e-4)
    assert one["q"][0, 0] == np.float64(np.float32(0.7))                      # a 1 x 1 image: Sigma = 0, c = 0, a = 0, b = p
    p = R.make_p("uniform", 9, 11, 3)
    flat = R.guided_filter(np.full((9, 11, 3), 0.5, np.float32), p, 2, 1e-4)  # a constant guide: a = 0, q = mean of mean of p
    mm = R.window_means(R.window_means(p.astype(np.float64)[:, :, None], 2), 2)[:, :, 0]
    assert np.abs(flat["q"] - mm).max() < 1e-10
    for C in (1, 3):                                                          # p constant: c = 0, q = p
        ref = R.guided_filter(R.make_guide("uniform", 9, 11, C, 5), np.full((9, 11), 0.25, np.float32), 3, 1e-6)
        assert (np.abs(ref["q"] - 0.25) <= R.q_bound(ref)).all()


def test_the_definition_does_its_job_on_the_disc_case():
    """DESIGN.md 10i's table, on the reference alone: the IoU of q > 0.5 against the disc."""
    _, p, disc = R.disc_case()
    assert abs(R.iou(p > 0.5, disc) - 0.823) < 1e-3
    for guide, r, eps, want in (("rgb", 8, 1e-4, 0.954), ("rgb", 16, 1e-6, 0.975), ("gray", 8, 1e-4, 0.873)):
        got = R.iou(_disc(guide, r, eps)["q"] > 0.5, disc)
        print(f"disc case {guide} r = {r} eps = {eps}: IoU {got:.4f}")
        assert abs(got - want) < 1e-3, (guide, r, eps, got)
    wide = _disc("rgb", 16, 1e-6)["q"]
    assert wide.min() < -0.05 and wide.max() > 1.05                           # the clamp has something to do (about -0.11 .. 1.07)


# ---- CPU: the binding and the host checks ------------------------------------------------------------------------------------------
def test_header_symbols_and_exports():
    from camouflage_multimodal_amd import _lib
    text = open(os.path.join(ROOT, "include", "camo_guided.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = re.findall(r"\b(camo_guided_[a-z_]+)\s*\(", code)
    assert tuple(names) == _lib.symbols("camo_guided.h") == ("camo_guided_workspace_bytes", "camo_guided_filter", "camo_guided_apply")
    assert "struct" not in code
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n)
    macros = dict(re.findall(r"#define (CAMO_GF_\w+) (\S+)", code))
    assert int(macros["CAMO_GF_MAX_RADIUS"]) == _lib.GF_MAX_RADIUS and int(macros["CAMO_GF_FIELDS"]) == _lib.GF_FIELDS
    assert float(macros["CAMO_GF_MIN_EPS"]) == _lib.GF_MIN_EPS and float(macros["CAMO_GF_MAX_EPS"]) == _lib.GF_MAX_EPS
    assert _lib.ABI_VERSION == 13


def test_host_argument_checks_need_no_device():
    """Every refused call returns CAMO_E_ARG before any launch: the pointers below are never dereferenced."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    N, H, W, C = 2, 5, 7, 3
    need = L.camo_guided_workspace_bytes(N, H, W, C)
    assert need >= N * H * W * 17 * 8 and L.camo_guided_workspace_bytes(N, H, W, 1) >= N * H * W * 6 * 8
    for bad in ((0, H, W, C), (N, 0, W, C), (N, H, 0, C), (N, H, W, 2), (N, H, W, 4), (65536, H, W, C), (1, 8193, 1, C), (1, 8192, 8193, C)):
        assert L.camo_guided_workspace_bytes(*bad) == 0, bad
    ptr = 0x10000                                                              # 256-byte aligned, never touched
    good = dict(guide=ptr, p=ptr, stride=H * W, N=N, H=H, W=W, C=C, radius=8, eps=1e-4, clamp=1, q=ptr, coef=ptr, ws=ptr, ws_bytes=need)

    def filt(**kw):
        a = {**good, **kw}
        return L.camo_guided_filter(a["guide"], a["p"], a["stride"], a["N"], a["H"], a["W"], a["C"], a["radius"], a["eps"], a["clamp"], a["q"],
                                    a["coef"], a["ws"], a["ws_bytes"], None)
    for kw in (dict(radius=0), dict(radius=65), dict(eps=0.0), dict(eps=5e-7), dict(eps=2.0), dict(eps=float("nan")), dict(C=2), dict(guide=None),
               dict(p=None), dict(q=None), dict(ws=None), dict(stride=H * W - 1), dict(ws=ptr + 8), dict(ws_bytes=need - 1), dict(clamp=2),
               dict(N=0), dict(H=0), dict(q=ptr + 2), dict(coef=ptr + 1)):
        assert filt(**kw) == E_ARG, kw
        assert L.camo_last_error()

    agood = dict(coef=ptr, N=N, C=C, h=H, w=W, guide=ptr, guide_elems=100, out=ptr, out_elems=100, table=ptr, mdp=35, clamp=1, status=ptr)

    def apply(**kw):
        a = {**agood, **kw}
        return L.camo_guided_apply(a["coef"], a["N"], a["C"], a["h"], a["w"], a["guide"], a["guide_elems"], a["out"], a["out_elems"], a["table"],
                                   a["mdp"], a["clamp"], a["status"], None)
    for kw in (dict(coef=None), dict(guide=None), dict(out=None), dict(table=None), dict(status=None), dict(C=2), dict(N=0), dict(h=0), dict(w=8193),
               dict(guide_elems=0), dict(out_elems=0), dict(mdp=0), dict(mdp=(1 << 26) + 1), dict(clamp=-1), dict(table=ptr + 4), dict(out=ptr + 2),
               dict(status=ptr + 1)):
        assert apply(**kw) == E_ARG, kw


def test_refine_raises_on_cpu_tensors_and_bad_shapes():
    from camouflage_multimodal_amd import _lib, refine
    g, p = torch.zeros(2, 5, 7, 3), torch.zeros(2, 5, 7)
    with pytest.raises(_lib.CamoError):
        refine.guided_filter(g, p)
    with pytest.raises(_lib.CamoError):
        refine.guided_upsample(torch.zeros(1, 4, 5, 7), [np.zeros((9, 9, 3), np.uint8)])
    for gg, pp in ((g, torch.zeros(2, 5, 8)), (g[:1], p), (torch.zeros(2, 5, 7, 2), p), (g, torch.zeros(5, 7)), (torch.zeros(5, 7, 3, 1), torch.zeros(5, 7))):
        with pytest.raises(ValueError):
            refine.guided_filter(gg, pp)
    for kw in (dict(radius=0), dict(radius=65), dict(radius=2.5), dict(eps=0.0), dict(eps=5e-7), dict(eps=2.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            refine.guided_filter(g, p, **kw)
    for bad in ("yes", dict(radius=0), dict(guide="hsv"), dict(window=3)):
        with pytest.raises(ValueError):
            refine.refine_options(bad)
    assert refine.refine_options(None) is None and refine.refine_options(True) == dict(radius=8, eps=1e-4, guide="rgb")
    assert refine.refine_options(dict(radius=16, guide="gray")) == dict(radius=16, eps=1e-4, guide="gray")


# ---- GPU: the filter ----------------------------------------------------------------------------------------------------------------------
def _within(name, got, ref, bound):
    frac = float((np.abs(got.astype(np.float64) - ref) / bound).max())
    print(f"{name}: max error / bound = {frac:.3f}")
    assert np.isfinite(got).all() and frac <= 1.0, (name, frac)
    return frac


def _run_filter(guide, p, r, eps, clamp=False, coefficients=True, in_place=True):
    """``p`` goes in as channel 0 of a [N, 3, H, W] map unless ``in_place`` is off."""
    from camouflage_multimodal_amd import guided_filter
    pt = torch.from_numpy(p).cuda()
    if in_place:
        maps = torch.full((p.shape[0], 3) + p.shape[1:], 7.0, device="cuda")
        maps[:, 0] = pt
        pt = maps[:, 0]
    out = guided_filter(torch.from_numpy(guide).cuda(), pt, r, eps, clamp, coefficients)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if coefficients else out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(FILTER_CASES)))
def test_filter_against_the_reference(i):
    (H, W), r, C, eps, gk, pk, N = FILTER_CASES[i]
    guide, p, refs = _filter_case(i)
    q, coef = _run_filter(guide, p, r, eps)
    assert q.shape == (N, H, W) and coef.shape == (N, C + 1, H, W) and q.dtype == coef.dtype == np.float32
    for n, ref in enumerate(refs):
        _within(f"q {FILTER_CASES[i]} image {n}", q[n], ref["q"], R.q_bound(ref))
        _within(f"coef {FILTER_CASES[i]} image {n}", coef[n], ref["coef"], R.coef_bounds(ref))
    again_q, again_coef = _run_filter(guide, p, r, eps)
    assert again_q.tobytes() == q.tobytes() and again_coef.tobytes() == coef.tobytes()              # two calls, the same bytes
    assert _run_filter(guide, p, r, eps, coefficients=False).tobytes() == q.tobytes()               # coef = null: the same q
    assert _run_filter(guide, p, r, eps, in_place=False)[0].tobytes() == q.tobytes()                # a contiguous p: the same q
    if N > 1:                                                                                       # a batch is its images one by one
        for n in range(N):
            q1, c1 = _run_filter(guide[n:n + 1], p[n:n + 1], r, eps)
            assert q1[0].tobytes() == q[n].tobytes() and c1[0].tobytes() == coef[n].tobytes()
    if H * W == 1:
        assert q[0, 0, 0] == p[0, 0, 0]


@pytest.mark.gpu
def test_filter_single_image_forms_and_grey_guide():
    from camouflage_multimodal_amd import guided_filter
    guide, p, refs = _filter_case(9)
    g, pt = torch.from_numpy(guide[0]).cuda(), torch.from_numpy(p[0]).cuda()
    q = guided_filter(g, pt, 8, 1e-4, clamp=False)
    assert tuple(q.shape) == (1, 64, 96)
    _within("single image", q[0].cpu().numpy(), refs[0]["q"], R.q_bound(refs[0]))
    grey = R.grey(guide[0])
    ref = R.guided_filter(grey, p[0], 8, 1e-4)
    a = guided_filter(torch.from_numpy(grey).cuda(), pt, 8, 1e-4, clamp=False)                       # [H, W] guide with [H, W] p
    b = guided_filter(torch.from_numpy(grey[None]).cuda(), pt[None], 8, 1e-4, clamp=False)           # [N, H, W] guide
    c = guided_filter(torch.from_numpy(grey[None, :, :, None]).cuda(), pt[None], 8, 1e-4, clamp=False)
    assert torch.equal(a, b) and torch.equal(a, c)
    _within("grey guide", a[0].cpu().numpy(), ref["q"], R.q_bound(ref))


@pytest.mark.gpu
def test_filter_clamp_and_the_disc_case_on_the_device():
    img, p, disc = R.disc_case()
    wide = _disc("rgb", 16, 1e-6)
    assert wide["q"].min() < 0 and wide["q"].max() > 1
    free, _ = _run_filter(img[None], p[None], 16, 1e-6, clamp=False)
    _within("disc r = 16 eps = 1e-6", free[0], wide["q"], R.q_bound(wide))
    clamped, coef = _run_filter(img[None], p[None], 16, 1e-6, clamp=True)
    assert clamped.min() == 0.0 and clamped.max() == 1.0
    _within("the same, clamped", clamped[0], np.clip(wide["q"], 0, 1), R.q_bound(wide))
    _within("its coefficients", coef[0], wide["coef"], R.coef_bounds(wide))
    q, _ = _run_filter(img[None], p[None], 8, 1e-4, clamp=True)
    got, painted = R.iou(q[0] > 0.5, disc), R.iou(p > 0.5, disc)
    print(f"disc case on the device (rgb, 8, 1e-4): IoU {got:.4f}, painted {painted:.4f}")
    assert got >= 0.90 and got >= painted + 0.05


# ---- GPU: the apply -----------------------------------------------------------------------------------------------------------------------
def _coef(N, C, h, w, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-8, 8, (N, C + 1, h, w)).astype(np.float32)


def _images(sizes, C, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (H, W, C) if C > 1 else (H, W)).astype(np.uint8) for H, W in sizes]


def _check_apply(name, coef, images, clamp=False):
    from camouflage_multimodal_amd import guided_upsample
    views, buf = guided_upsample(torch.from_numpy(coef).cuda(), images, clamp)
    assert buf.numel() == sum(im.shape[0] * im.shape[1] for im in images) and buf.dtype == torch.float32
    for i, (v, im) in enumerate(zip(views, images)):
        assert tuple(v.shape) == im.shape[:2]
        ref, terms = R.guided_apply(coef[i], im, clamp)
        _within(f"{name} image {i} {coef.shape[2:]} -> {im.shape[:2]}", v.cpu().numpy(), ref, np.maximum(R.apply_bound(ref, terms), 1e-300))
    return views, buf


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 3))
def test_apply_against_the_reference(C):
    for k, ((h, w), (H, W)) in enumerate((((1, 1), (1, 1)), ((3, 5), (40, 33)), ((33, 70), (7, 9)))):      # downwards is legal
        _check_apply("apply", _coef(1, C, h, w, 10 * k + C), _images([(H, W)], C, k))
    sizes = [(40, 33), (7, 9), (1, 1), (65, 130)]                                                       # ragged; 65 x 130 is more than one block a row
    coef, images = _coef(4, C, 12, 20, 50 + C), _images(sizes, C, 60 + C)
    views, buf = _check_apply("ragged", coef, images)
    _check_apply("ragged, clamped", coef, images, clamp=True)
    from camouflage_multimodal_amd import guided_upsample
    assert guided_upsample(torch.from_numpy(coef).cuda(), images, False)[1].cpu().numpy().tobytes() == buf.cpu().numpy().tobytes()
    for i, im in enumerate(images):                                                                     # batch = rows
        one, _ = guided_upsample(torch.from_numpy(coef[i:i + 1]).cuda(), [im], False)
        assert one[0].cpu().numpy().tobytes() == views[i].cpu().numpy().tobytes()
    stacked = torch.from_numpy(np.stack([images[0]] * 2)).cuda()                                        # a uint8 [N, H, W(, C)] tensor is a ragged batch too
    two, _ = guided_upsample(torch.from_numpy(coef[:2]).cuda(), stacked, False)
    assert torch.equal(two[0], views[0])


@pytest.mark.gpu
def test_apply_working_size_to_a_native_size():
    _check_apply("256^2 -> 600 x 800", _coef(1, 3, 256, 256, 5), _images([(600, 800)], 3, 6))


@pytest.mark.gpu
def test_apply_refuses_a_bad_row_and_leaves_its_neighbours():
    from camouflage_multimodal_amd import pack_images
    from camouflage_multimodal_amd.refine import guided_apply_table, guided_upsample
    C, sizes = 3, [(9, 11), (6, 5), (8, 8), (4, 7)]
    coef, images = _coef(4, C, 5, 6, 70), _images(sizes, C, 71)
    packed = pack_images(images)
    good_views, _ = guided_upsample(torch.from_numpy(coef).cuda(), packed, False)
    offs, outs, at = packed.offsets(), [], 0
    for H, W in sizes:
        outs.append(at)
        at += H * W
    rows = [[offs[i], H, W, outs[i]] for i, (H, W) in enumerate(sizes)]
    rows[1][0] = packed.data.numel() - 10                       # the guide footprint leaves the buffer: status 1, zeros
    rows[2][1] = 0                                              # a side of 0: status 1, nothing stored
    out = torch.full((at,), 7.0, device="cuda")
    status = guided_apply_table(torch.from_numpy(coef).cuda(), packed.data, out, torch.tensor(rows, dtype=torch.int64).cuda(), 99, False)
    assert status.tolist() == [0, 1, 1, 0]
    got = out.cpu().numpy()
    for i in (0, 3):
        H, W = sizes[i]
        assert got[outs[i]:outs[i] + H * W].tobytes() == good_views[i].cpu().numpy().tobytes()
    assert (got[outs[1]:outs[1] + 30] == 0).all() and (got[outs[2]:outs[2] + 64] == 7.0).all()
    rows[3][3] = at - 10                                        # the destination leaves the buffer: zeros over the part inside it only
    out = torch.full((at,), 7.0, device="cuda")
    status = guided_apply_table(torch.from_numpy(coef).cuda(), packed.data, out, rows, 99, False)
    assert status.tolist() == [0, 1, 1, 1]
    got = out.cpu().numpy()
    assert (got[at - 10:] == 0).all() and (got[outs[3]:at - 10] == 7.0).all()
    assert got[:99].tobytes() == good_views[0].cpu().numpy().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 3))
def test_apply_is_resize_then_multiply_add(C):
    """``guided_upsample`` against ``resize_to_sizes`` of the coefficient planes followed by the multiply-add in float64 on the host.
    ``resize_to_sizes`` rounds every sample to fp32, which the apply does not; so that the two can be held to the apply's own bound the
    coefficients are multiples of 2^-6 in [-8, 8] and the sizes give a power-of-two den (4 x 8 -> 16 x 32: den = 2^11): every sample is
    a multiple of 2^-17 below 8 in magnitude, 20 bits, exact in fp32."""
    from camouflage_multimodal_amd import guided_upsample, resize_to_sizes
    rs = np.random.RandomState(80 + C)
    coef = (rs.randint(-512, 513, (2, C + 1, 4, 8)) / 64.0).astype(np.float32)
    sizes = [(16, 32), (8, 8)]
    images = _images(sizes, C, 81)
    views, _ = guided_upsample(torch.from_numpy(coef).cuda(), images, False)
    planes, _ = resize_to_sizes(torch.from_numpy(coef).cuda(), sizes, "bilinear")
    for i, (v, im) in enumerate(zip(views, images)):
        up = planes[i].cpu().numpy().astype(np.float64)
        g = (im if C > 1 else im[:, :, None]).astype(np.float64) / 255.0
        t = up[:C].transpose(1, 2, 0) * g
        ref = t.sum(axis=2) + up[C]
        _within(f"composition image {i}", v.cpu().numpy(), ref, np.maximum(R.apply_bound(ref, np.abs(t).sum(axis=2) + np.abs(up[C])), 1e-300))
        direct, _ = R.guided_apply(coef[i], im)
        assert np.abs(direct - ref).max() <= 2.0 ** -45 * 40
