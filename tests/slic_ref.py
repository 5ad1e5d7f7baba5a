"""numpy / scipy.ndimage restatement of the SLIC label map of include/camo_slic.h (steps 1-8 there), the checker of
tests/test_slic.py.  PARITY UNPINNED: scikit-image is not importable here; the header's text is the definition (the published
skimage.segmentation.slic with the reference's arguments and two stated deviations) and this file follows it step by step.

Every stage runs in the dtype asked for, one rounding per operation in the header's order, so that the float32 evaluation of
``assign`` and ``update`` is what the device must reproduce bit for bit, and the float64 one is the yardstick of everything else.
The connectivity step is the plain sequential loop, with skimage's cut at ``max_size`` behind a switch.
"""
import math

import numpy as np

import canny_ref as CR

ITERATIONS = 10
FIX = 2.0 ** 24
NEIGHBOURS = ((0, 1), (0, -1), (1, 0), (-1, 0))          # +x, -x, +y, -y


# ---- steps 1-3 -----------------------------------------------------------------------------------------------------------

def quantise(image, dtype=np.float64):
    """Step 1: fp32 image -> v = q / 255 in ``dtype`` (q is computed in fp32 in either case: the input is fp32)."""
    q = np.clip(np.trunc(np.asarray(image, np.float32) * np.float32(255.0)), 0, 255)
    return q.astype(dtype) / dtype(255)


def gaussian_weights(sigma):
    if sigma == 0:
        return np.ones(1)
    return CR.gaussian_weights(sigma)


def reflect_index(i, n):
    """scipy.ndimage mode="reflect": d c b a | a b c d | d c b a."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def smooth(v, sigma=1.0, dtype=np.float64):
    """Step 2 on [H, W, C]: along x, then along y."""
    w = gaussian_weights(sigma).astype(dtype)
    r = len(w) // 2
    out = np.asarray(v).astype(dtype)
    for axis in (1, 0):
        n = out.shape[axis]
        p = np.take(out, reflect_index(np.arange(-r, n + r), n), axis=axis)
        acc = np.zeros_like(out)
        for k in range(len(w)):
            acc = acc + w[k] * np.take(p, np.arange(k, k + n), axis=axis)
        out = acc
    return out


def lab_scaled(v, compactness=10.0, dtype=np.float64):
    """Step 3 on [..., 3]."""
    t = dtype
    v = np.asarray(v).astype(t)
    lin = np.where(v > t(0.04045), np.power((v + t(0.055)) / t(1.055), t(2.4)), v / t(12.92))
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    x = ((r * t(0.412453) + g * t(0.357580)) + b * t(0.180423)) / t(0.95047)
    y = (r * t(0.212671) + g * t(0.715160)) + b * t(0.072169)
    z = ((r * t(0.019334) + g * t(0.119193)) + b * t(0.950227)) / t(1.08883)

    def f(u):
        return np.where(u > t(0.008856), np.cbrt(u), t(7.787) * u + t(16) / t(116))
    fx, fy, fz = f(x), f(y), f(z)
    inv = t(1) / t(np.float32(compactness))
    return np.stack([(t(116) * fy - t(16)) * inv, (t(500) * (fx - fy)) * inv, (t(200) * (fy - fz)) * inv], -1).astype(t)


def preprocess(image, compactness=10.0, sigma=1.0, dtype=np.float64):
    return lab_scaled(smooth(quantise(image, dtype), sigma, dtype), compactness, dtype)


# ---- step 4 --------------------------------------------------------------------------------------------------------------

def grid(H, W, n_segments):
    """-> dict K, step, start, ny, nx; ValueError where the header refuses."""
    if H < 1 or W < 1 or n_segments < 1:
        raise ValueError("need H, W, n_segments >= 1")
    if H * W <= n_segments:
        raise ValueError("need H W > n_segments")
    s = math.sqrt(H * W / n_segments)
    if min(H, W) < s:
        raise ValueError("need min(H, W) >= s")
    step, start = int(round(s)), int(math.floor(s / 2))               # (Python's round is half-even)
    ny, nx = -(-(H - start) // step), -(-(W - start) // step)
    return dict(K=ny * nx, step=step, start=start, ny=ny, nx=nx)


def initial_centroids(g, dtype=np.float64):
    c = np.zeros((g["K"], 5), dtype)
    k = np.arange(g["K"])
    c[:, 0] = g["start"] + (k // g["nx"]) * g["step"]
    c[:, 1] = g["start"] + (k % g["nx"]) * g["step"]
    return c


# ---- steps 5-7 -----------------------------------------------------------------------------------------------------------

def window(c, step, n, t):
    """Half-open candidate range along one axis of a centroid coordinate c, and whether each end comes from the truncation
    (not from the image border)."""
    two = t(2 * step)
    lo, hi = c - two, (c + two) + t(1)
    return int(max(lo, t(0))), int(min(hi, t(n))), bool(lo > 0), bool(hi < n)


def assign(lab, cent, step, dtype=np.float64):
    """Step 5 -> (nearest int32 [H, W], best, second, soft): best / second smallest distance per pixel (second = best on an
    exact tie, inf with fewer than two candidates); soft = the winner's window ends, by truncation, at the pixel's row or column."""
    t = dtype
    lab, cent = np.asarray(lab).astype(t), np.asarray(cent).astype(t)
    H, W = lab.shape[:2]
    w = t(1) / t(step * step)
    best = np.full((H, W), np.inf, t); second = np.full((H, W), np.inf, t)
    near = np.zeros((H, W), np.int32); soft = np.zeros((H, W), bool)
    for k in range(len(cent)):
        cy, cx = cent[k, 0], cent[k, 1]
        y0, y1, sy0, sy1 = window(cy, step, H, t)
        x0, x1, sx0, sx1 = window(cx, step, W, t)
        if y0 >= y1 or x0 >= x1:
            continue
        ey = cy - np.arange(y0, y1).astype(t)[:, None]; ex = cx - np.arange(x0, x1).astype(t)[None, :]
        px = lab[y0:y1, x0:x1]
        el, ea, eb = cent[k, 2] - px[..., 0], cent[k, 3] - px[..., 1], cent[k, 4] - px[..., 2]
        d = (ey * ey + ex * ex) * w + ((el * el + ea * ea) + eb * eb)
        b, s2 = best[y0:y1, x0:x1], second[y0:y1, x0:x1]
        win = d < b
        e = np.zeros(d.shape, bool)
        if sy0: e[0, :] = True
        if sy1: e[-1, :] = True
        if sx0: e[:, 0] = True
        if sx1: e[:, -1] = True
        second[y0:y1, x0:x1] = np.where(win, b, np.minimum(s2, d))
        best[y0:y1, x0:x1] = np.where(win, d, b)
        near[y0:y1, x0:x1] = np.where(win, k, near[y0:y1, x0:x1])
        soft[y0:y1, x0:x1] = np.where(win, e, soft[y0:y1, x0:x1])
    return near, best, second, soft


def update(lab, near, cent, dtype=np.float64):
    """Step 6.  float32: the device's sums (integers; colours as int64 in units of 2^-24); float64: plain float64 sums."""
    K = len(cent)
    H, W = near.shape
    flat = near.ravel().astype(np.int64)
    ok = (flat >= 0) & (flat < K)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cnt = np.bincount(flat[ok], minlength=K)
    new = np.array(cent, dtype)
    has = cnt > 0
    n = cnt[has].astype(np.float64)
    for j, coord in enumerate((yy, xx)):
        s = np.zeros(K, np.int64); np.add.at(s, flat[ok], coord.ravel()[ok])
        new[has, j] = (s[has].astype(np.float64) / n).astype(dtype)
    for j in range(3):
        c = np.asarray(lab)[..., j].ravel()[ok]
        if dtype == np.float32:
            s = np.zeros(K, np.int64); np.add.at(s, flat[ok], np.rint(c.astype(np.float32) * np.float32(FIX)).astype(np.int64))
            new[has, 2 + j] = (s[has].astype(np.float64) / (n * FIX)).astype(np.float32)
        else:
            s = np.bincount(flat[ok], weights=c.astype(np.float64), minlength=K)
            new[has, 2 + j] = s[has] / n
    return new


def iterate(lab, g, dtype=np.float64):
    """Step 7 -> list of ITERATIONS records dict(cent = centroids going into the assign, near, best, second, soft)."""
    cent = initial_centroids(g, dtype)
    out = []
    for _ in range(ITERATIONS):
        near, best, second, soft = assign(lab, cent, g["step"], dtype)
        out.append(dict(cent=cent, near=near, best=best, second=second, soft=soft))
        cent = update(lab, near, cent, dtype)
    return out


# ---- step 8 --------------------------------------------------------------------------------------------------------------

def sizes(H, W, K):
    seg = H * W / K
    return int(0.5 * seg), int(3 * seg)


def connect(seg, min_size, max_size, cut=False):
    """The sequential relabelling -> (labels int32 [H, W], components of >= max_size pixels).  cut=True stops a search at
    max_size pixels as skimage does (the rest of the component is then met again as a new one); the device does not."""
    seg = np.asarray(seg)
    H, W = seg.shape
    out = np.full((H, W), -1, np.int32)
    stamp = np.zeros((H, W), np.int64)
    new, over, ident = 1, 0, 0
    for y in range(H):
        for x in range(W):
            if out[y, x] >= 0:
                continue
            ident += 1
            comp = [(y, x)]; stamp[y, x] = ident
            adjacent, i, stop = 0, 0, False
            while i < len(comp) and not stop:
                cy, cx = comp[i]; i += 1
                for dy, dx in NEIGHBOURS:
                    ny, nx = cy + dy, cx + dx
                    if ny < 0 or ny >= H or nx < 0 or nx >= W:
                        continue
                    if seg[ny, nx] == seg[y, x] and out[ny, nx] < 0:
                        if stamp[ny, nx] != ident:
                            stamp[ny, nx] = ident; comp.append((ny, nx))
                            if cut and len(comp) >= max_size:
                                stop = True
                                break
                    elif out[ny, nx] >= 0:
                        adjacent = out[ny, nx]
            over += len(comp) >= max_size
            label = adjacent
            if len(comp) >= min_size:
                label = new; new += 1
            for cy, cx in comp:
                out[cy, cx] = label
    return out, over


def slic(image, n_segments, compactness=10.0, sigma=1.0, dtype=np.float64, cut=False):
    """-> (labels int32 [H, W], oversized components, the records of ``iterate``)."""
    H, W = np.asarray(image).shape[:2]
    g = grid(H, W, n_segments)
    rec = iterate(preprocess(image, compactness, sigma, dtype), g, dtype)
    labels, over = connect(rec[-1]["near"] + 1, *sizes(H, W, g["K"]), cut=cut)
    return labels, over, rec


def four_connected(labels, ignore=()):
    """Every label (outside ``ignore``) forms one 4-connected component."""
    from scipy import ndimage
    for v in np.unique(labels):
        if v in ignore:
            continue
        if ndimage.label(labels == v)[1] != 1:
            return False
    return True


# ---- seeded inputs ------------------------------------------------------------------------------------------------------

def blob_image(H, W, seed):
    return CR.colour_image(H, W, seed)


def noise_image(H, W, seed):
    """Uniform noise per channel on top of a blob field: texture with structure under it."""
    rs = np.random.RandomState(seed)
    return np.clip(0.6 * CR.colour_image(H, W, seed + 100) + 0.4 * rs.uniform(0, 1, (H, W, 3)), 0, 1).astype(np.float32)


TABLE = {"20x28": (20, 28, 12, (7, 3, 3, 4, 12)), "33x70": (33, 70, 40, (8, 3, 4, 9, 36)), "96x80": (96, 80, 60, (11, 5, 9, 7, 63)),
         "256x256": (256, 256, 500, (11, 5, 23, 23, 529))}          # H, W, n_segments, (step, start, ny, nx, K)
CLEAR = ("20x28", "33x70", "96x80")
SEEDS = {"20x28": (("blob", 0), ("noise", 0)), "33x70": (("blob", 3), ("noise", 14)), "96x80": (("blob", 3963), ("noise", 447)),
         "256x256": (("blob", 3), ("noise", 4))}


def cases():
    """name -> (float32 images [N, H, W, 3], n_segments) at the four shapes of the header's table: blob fields and noise over
    blob fields (canny_ref's fields; flat Voronoi levels are not used: they tie).  The seeds of the three small cases are chosen
    with this reference alone: in the float64 run every margin second - best of every iteration is an exact tie of iteration 0
    or at least 2.2e-4 (test_slic.TAU is 2e-4; a few thousand seeds were tried for 96 x 80), no winner's window ends at the pixel's row or column, and the float32 run gives
    the float64 labels.  256 x 256 is not held to that: with 650 000 margins some lie below any usable bound."""
    out = {}
    for name, (H, W, n, _) in TABLE.items():
        out[name] = (np.stack([(blob_image if kind == "blob" else noise_image)(H, W, seed) for kind, seed in SEEDS[name]]), n)
    return out
