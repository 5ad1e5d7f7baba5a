"""numpy restatement of include/camo_augment.h (PARITY UNPINNED: the header's text is the definition; this file shares no code with
the package).  Everything is integer arithmetic in int64 -- numpy's // and >> are floors, also of negative values -- so callers
compare for equality.
"""
import numpy as np

NEAREST, BILINEAR = "nearest", "bilinear"
FIELDS = 24
F = 16
MAX_SIDE = 8192


def warp(img, size, clip, mat, border=0, fill=0, mode=BILINEAR, out="u8"):
    """One uint8 image [H, W] or [H, W, C] through the inverse map ``mat`` = (a00, a01, b0, a10, a11, b1) to ``size`` = (Ho, Wo):
    uint8 (``out="u8"``) or float32 (``out="f32"``: num over 255 den).  ``clip`` = (y0, x0, h, w) is the part that may be read."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    squeeze = img.ndim == 2
    a = (img[:, :, None] if squeeze else img).astype(np.int64)
    H, W, C = a.shape
    Ho, Wo = size
    y0, x0, ch, cw = clip
    assert 0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= H and x0 + cw <= W and border in (0, 1)
    a00, a01, b0, a10, a11, b1 = (int(v) for v in mat)
    dy, dx = np.meshgrid(np.arange(Ho, dtype=np.int64), np.arange(Wo, dtype=np.int64), indexing="ij")
    X = a00 * (2 * dx + 1) + a01 * (2 * dy + 1) + b0
    Y = a10 * (2 * dx + 1) + a11 * (2 * dy + 1) + b1
    fillv = np.array([(int(fill) >> (8 * c)) & 255 for c in range(C)], np.int64)

    def tap(iy, ix):
        inside = (iy >= y0) & (iy < y0 + ch) & (ix >= x0) & (ix < x0 + cw)
        p = a[np.clip(iy, y0, y0 + ch - 1), np.clip(ix, x0, x0 + cw - 1)]           # [Ho, Wo, C]
        return p if border == 1 else np.where(inside[:, :, None], p, fillv[None, None, :])

    if mode == NEAREST:
        num, den = tap((Y + (1 << (F - 1))) >> F, (X + (1 << (F - 1))) >> F), 1
    else:
        assert mode == BILINEAR
        ix, iy = X >> F, Y >> F
        wx1, wy1 = X - (ix << F), Y - (iy << F)
        wx0, wy0 = (1 << F) - wx1, (1 << F) - wy1
        num = ((wy0 * wx0)[:, :, None] * tap(iy, ix) + (wy0 * wx1)[:, :, None] * tap(iy, ix + 1)
               + (wy1 * wx0)[:, :, None] * tap(iy + 1, ix) + (wy1 * wx1)[:, :, None] * tap(iy + 1, ix + 1))
        den = 1 << (2 * F)
    if out == "f32":
        res = (num.astype(np.float64) / np.float64(255 * den)).astype(np.float32)
    else:
        assert out == "u8"
        res = ((2 * num + den) // (2 * den)).astype(np.uint8)
    return res[:, :, 0] if squeeze else res


def blend(deg, v, k):
    return np.clip((deg * (256 - k) + v * k + 128) // 256, 0, 255)


def luma(p):
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16


def brightness(img, k):
    return blend(0, np.asarray(img).astype(np.int64), int(k)).astype(np.uint8)


def contrast(img, k):
    v = np.asarray(img).astype(np.int64)
    S, P = int(luma(v).sum()), v.shape[0] * v.shape[1]
    return blend((2 * S + P) // (2 * P), v, int(k)).astype(np.uint8)


def colour(img, k):
    v = np.asarray(img).astype(np.int64)
    return blend(luma(v)[..., None], v, int(k)).astype(np.uint8)


def sharpness(img, k):
    v = np.asarray(img).astype(np.int64)
    H, W = v.shape[:2]
    sm = v.copy()
    if H >= 3 and W >= 3:
        s = 4 * v[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                s = s + v[dy:dy + H - 2, dx:dx + W - 2]
        sm[1:-1, 1:-1] = (2 * s + 13) // 26
    return blend(sm, v, int(k)).astype(np.uint8)


def enhance(img, ks):
    """uint8 [Ho, Wo, 3] through brightness, contrast, colour, sharpness with the Q8 factors ``ks``, in that order."""
    kb, kc, kcol, kh = ks
    return sharpness(colour(contrast(brightness(img, kb), kc), kcol), kh)


def row_ok(r, C, src_elems, enhance_on, max_side=MAX_SIDE):
    """The header's row conditions, in Python integers."""
    r = [int(v) for v in r]
    so, sh, sw, srs, sps, scs, y0, x0, ch, cw = r[:10]
    ok = (len(r) == FIELDS and all(1 <= v <= max_side for v in (sh, sw, ch, cw)) and y0 >= 0 and x0 >= 0 and y0 + ch <= sh and x0 + cw <= sw
          and min(srs, sps, scs) >= 1 and so >= 0 and so + (sh - 1) * srs + (sw - 1) * sps + (C - 1) * scs < src_elems
          and all(abs(r[i]) <= 1 << 30 for i in (10, 11, 13, 14)) and all(abs(r[i]) <= 1 << 46 for i in (12, 15))
          and r[16] in (0, 1) and 0 <= r[17] < 1 << 32 and r[22] == 0 and r[23] == 0)
    return bool(ok and (not enhance_on or all(0 <= k <= 1024 for k in r[18:22])))


def run_table(src, table, C, size, mode, enhance_on, out):
    """What camo_augment leaves in dst ([N, Ho, Wo, C], ``out`` "u8" or "f32") and in status, for flat uint8 ``src`` and a [N, 24]
    table; a refused row leaves zeros."""
    Ho, Wo = size
    rows = np.asarray(table).tolist()
    dst = np.zeros((len(rows), Ho, Wo, C), np.uint8 if out == "u8" else np.float32)
    status = np.zeros(len(rows), np.int32)
    for i, r in enumerate(rows):
        if not row_ok(r, C, src.size, enhance_on):
            status[i] = 1
            continue
        so, sh, sw, srs, sps, scs = r[:6]
        sy, sx, sc = np.meshgrid(np.arange(sh), np.arange(sw), np.arange(C), indexing="ij")
        img = src[so + sy * srs + sx * sps + sc * scs]
        if not enhance_on:
            dst[i] = warp(img, size, r[6:10], r[10:16], r[16], r[17], mode, out)
        else:
            v = enhance(warp(img, size, r[6:10], r[10:16], r[16], r[17], mode, "u8"), r[18:22])
            dst[i] = v if out == "u8" else (v.astype(np.float64) / np.float64(255.0)).astype(np.float32)
    return dst, status
