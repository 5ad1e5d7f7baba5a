"""numpy / scipy.ndimage restatement of the Canny edge map of include/camo_canny.h (steps 1-5 there), the checker of
tests/test_canny.py.  PARITY UNPINNED: scikit-image is not importable here; this is its published algorithm
(skimage.feature.canny: Gaussian smoothing with mask normalisation, scipy.ndimage.sobel, bilinear non-maximum suppression in
four angle classes, double threshold, 8-connected hysteresis with ndimage.label) with the reference's arguments.

Every stage runs in the dtype asked for, one rounding per operation, so that the float32 evaluation of ``decide`` is what the
device's fp32 decision stage must reproduce bit for bit, and the float64 one is the yardstick of everything else.
"""
import numpy as np
from scipy import ndimage

LUMA = (0.2989, 0.5870, 0.1140)
EPS = 2.0 ** -52
ALL8 = np.ones((3, 3), bool)


def luma(image, dtype=np.float64):
    im = np.asarray(image).astype(dtype)
    return im[..., 0] * dtype(LUMA[0]) + im[..., 1] * dtype(LUMA[1]) + im[..., 2] * dtype(LUMA[2])


def gaussian_weights(sigma):
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * k * k)
    return phi / phi.sum()


def _blur(a, w, axis):
    """sum_k w[k] a[i + k - r] along ``axis``, zero outside."""
    r = len(w) // 2
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad)
    out = np.zeros_like(a)
    for k in range(len(w)):
        out += w[k] * np.take(p, np.arange(k, k + n), axis=axis)
    return out


def stage_a(gray, dtype=np.float64, sigma=2.0):
    """Steps 2-3: -> (gi, gj, m) in ``dtype``."""
    g = np.asarray(gray).astype(dtype)
    w = gaussian_weights(sigma).astype(dtype)
    H, W = g.shape
    sm = _blur(_blur(g, w, 1), w, 0)
    rf, cf = _blur(np.ones(H, dtype), w, 0), _blur(np.ones(W, dtype), w, 0)
    sm = sm / (rf[:, None] * cf[None, :] + dtype(EPS))
    p = np.pad(sm, 1, mode="edge")
    two = dtype(2)
    gi = (p[2:, :-2] + two * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + two * p[:-2, 1:-1] + p[:-2, 2:])
    gj = (p[:-2, 2:] + two * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + two * p[1:-1, :-2] + p[2:, :-2])
    return gi, gj, np.sqrt(gi * gi + gj * gj)


def stage_a_ndimage(gray, sigma=2.0):
    """The same two steps as scikit-image composes them from scipy.ndimage (float64)."""
    g = np.asarray(gray, np.float64)
    sm = ndimage.gaussian_filter(g, sigma, mode="constant") / (ndimage.gaussian_filter(np.ones_like(g), sigma, mode="constant") + EPS)
    gi, gj = ndimage.sobel(sm, axis=0), ndimage.sobel(sm, axis=1)
    return gi, gj, np.sqrt(gi * gi + gj * gj)


def suppression_terms(gi, gj, m):
    """Step 4's two comparisons for every pixel, in the dtype of the inputs: (forward, backward, m * b, b); a pixel is a local
    maximum when forward <= m * b and backward <= m * b.  m outside the image counts as 0."""
    H, W = m.shape
    s = np.where(((gi > 0) & (gj > 0)) | ((gi < 0) & (gj < 0)) | (gi == 0) | (gj == 0), 1, -1)
    ai, aj = np.abs(gi), np.abs(gj)
    steep = ai >= aj
    a, b = np.where(steep, aj, ai), np.where(steep, ai, aj)
    mp = np.pad(m, 1)
    r, c = np.meshgrid(np.arange(1, H + 1), np.arange(1, W + 1), indexing="ij")
    f1 = np.where(steep, mp[r + 1, c], mp[r, c + s]); f2 = mp[r + 1, c + s]
    b1 = np.where(steep, mp[r - 1, c], mp[r, c - s]); b2 = mp[r - 1, c - s]
    d = b - a
    return f2 * a + f1 * d, b2 * a + b1 * d, m * b, b


def interior(shape):
    k = np.zeros(shape, bool)
    k[1:-1, 1:-1] = True
    return k


def classes(gi, gj, m, low, high):
    """uint8 [H, W]: 0 none, 1 weak, 2 strong (thresholds rounded to the dtype of m, as the device holds them in fp32)."""
    t = m.dtype.type
    fwd, bwd, rhs, _ = suppression_terms(gi, gj, m)
    weak = interior(m.shape) & (fwd <= rhs) & (bwd <= rhs) & (m >= t(low))
    return weak.astype(np.uint8) + (weak & (m >= t(high)))


def hysteresis(cls):
    """Step 5: weak pixels whose 8-connected component of weak pixels holds a strong one."""
    lab, _ = ndimage.label(cls > 0, structure=ALL8)
    keep = np.zeros(lab.max() + 1, bool)
    keep[lab[cls > 1]] = True
    keep[0] = False
    return keep[lab]


def decide(gi, gj, m, low=0.1, high=0.2):
    return hysteresis(classes(gi, gj, m, low, high))


def canny(image, dtype=np.float64, sigma=2.0, low=0.1, high=0.2):
    """-> (edges bool [H, W], (gi, gj, m))."""
    g = stage_a(luma(image, dtype), dtype, sigma)
    return decide(*g, low, high), g


def excluded_components(g64, ref_cls, other_edges, tau, low=0.1, high=0.2):
    """bool [H, W]: the 8-connected components of (reference weak | the other map's edges | undecided pixels) that hold an
    undecided pixel.  Undecided, for gradients known to ``tau``: an interior pixel with m >= low - tau whose m is within tau
    of a threshold or one of whose two suppression comparisons is within tau * b of equality (float64 quantities)."""
    gi, gj, m = g64
    fwd, bwd, rhs, b = suppression_terms(gi, gj, m)
    near = (np.abs(m - low) <= tau) | (np.abs(m - high) <= tau) | (np.abs(fwd - rhs) <= tau * b) | (np.abs(bwd - rhs) <= tau * b)
    und = interior(m.shape) & (m >= low - tau) & near
    lab, _ = ndimage.label((ref_cls > 0) | other_edges | und, structure=ALL8)
    bad = np.zeros(lab.max() + 1, bool)
    bad[lab[und]] = True
    bad[0] = False
    return bad[lab]


# ---- seeded inputs ----------------------------------------------------------------------------------------------------

def voronoi_field(H, W, cells, seed):
    """Nearest-seed cells, each one of 12 flat grey levels."""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(0, 1, (cells, 2)) * (H, W)
    lev = rs.permutation(12)[np.arange(cells) % 12] / 11.0
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return lev[((yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2).argmin(-1)]


def blob_field(H, W, seed):
    """Six Gaussian blobs (3 to 8 pixels wide, alternating sign) on a mid-grey ground."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = np.full((H, W), 0.5)
    for k in range(6):
        cy, cx, s = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(3.0, 8.0)
        f += (0.5 if k % 2 else -0.5) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return np.clip(f, 0, 1)


def noise_field(H, W, seed):
    return np.random.RandomState(seed).uniform(0, 1, (H, W))


def grey_image(field):
    return np.repeat(np.asarray(field, np.float32)[..., None], 3, axis=-1)


def colour_image(H, W, seed):
    """A different blob field in each channel."""
    return np.stack([blob_field(H, W, seed), blob_field(H, W, seed + 1), blob_field(H, W, seed + 2)], -1).astype(np.float32)


def cases():
    """name -> float32 images [N, H, W, 3]: the shapes of the GPU tests.  The seeds are chosen with this reference alone: at
    tau = 1e-5 (gradients known to 2.5e-6, twice the error of this file's own float32 evaluation) the excluded share of every
    image is under 5 %.  Two things make other seeds unfit for a cap per connected component: where a border of two flat Voronoi
    levels runs parallel to an axis for longer than the blur's support the two pixels that straddle it tie exactly, and the
    borders form one connected net; and an image of a few rings loses a fifth of its edge pixels to one near-tie."""
    return {
        "9x13": np.stack([grey_image(voronoi_field(9, 13, 3, 1))]),
        "33x70": np.stack([grey_image(blob_field(33, 70, 2))]),
        "48x64": np.stack([grey_image(noise_field(48, 64, 3))]),
        "3x96x80": np.stack([grey_image(voronoi_field(96, 80, 12, 8)), grey_image(blob_field(96, 80, 4)), grey_image(noise_field(96, 80, 6))]),
        "2x256x256": np.stack([colour_image(256, 256, 3), grey_image(blob_field(256, 256, 4))]),
    }
