"""numpy restatement of include/camo_resize.h (PARITY UNPINNED: the header's text is the definition; this file shares no code with
the package).  A u8 source goes through the per-axis integer weight MATRICES, num = Wy . img . Wx^T in int64; an fp32 source
through the one or four taps, summed in float64 in the header's order.  Everything is exact, so callers compare for equality.
"""
import numpy as np

NEAREST, BILINEAR, AREA = "nearest", "bilinear", "area"
FIELDS = 18


def axis_taps(c0, cs, D, flip, mode):
    """The header's taps of one axis: (idx [D, k] source indices, w [D, k] integer weights, T) with k = 1 (nearest) or 2 (bilinear,
    and an area axis that does not shrink); ``None`` for an area axis with cs > D, which has no fixed tap count."""
    d = np.arange(D, dtype=np.int64)
    dd = D - 1 - d if flip else d
    if mode == NEAREST:
        return (c0 + ((2 * dd + 1) * cs) // (2 * D))[:, None], np.ones((D, 1), np.int64), 1
    if mode == AREA and cs > D:
        return None
    n = (2 * dd + 1) * cs - D
    i0 = n // (2 * D)                                       # numpy's // is the floor
    w1 = n - i0 * 2 * D
    w0 = 2 * D - w1
    idx = np.stack([c0 + np.clip(i0, 0, cs - 1), c0 + np.clip(i0 + 1, 0, cs - 1)], 1)
    return idx, np.stack([w0, w1], 1), 2 * D


def axis_matrix(src_len, c0, cs, D, flip, mode):
    """(W int64 [D, src_len], T): W[d, s] = the total weight of source index s in destination index d."""
    W = np.zeros((D, src_len), np.int64)
    taps = axis_taps(c0, cs, D, flip, mode)
    if taps is None:
        d = np.arange(D, dtype=np.int64)
        dd = (D - 1 - d if flip else d)[:, None]
        j = np.arange(cs, dtype=np.int64)[None, :]
        w = np.minimum((dd + 1) * cs, (j + 1) * D) - np.maximum(dd * cs, j * D)
        W[:, c0:c0 + cs] = np.maximum(w, 0)
        return W, cs
    idx, w, T = taps
    for k in range(idx.shape[1]):
        np.add.at(W, (np.arange(D), idx[:, k]), w[:, k])
    return W, T


def resize(img, size, mode=BILINEAR, crop=None, flip=0, out="f32"):
    """One image [H, W] or [H, W, C], uint8 or float32, to ``size`` = (Ho, Wo).  A u8 source gives float32 (``out="f32"``: num over
    255 den) or uint8 (``out="u8"``: a half rounds up); an fp32 source gives float32 (nearest and bilinear only)."""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    a = img[:, :, None] if squeeze else img
    H, W, C = a.shape
    Ho, Wo = size
    y0, x0, ch, cw = (0, 0, H, W) if crop is None else crop
    assert 0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= H and x0 + cw <= W and 0 <= flip <= 3
    if a.dtype == np.uint8:
        Wy, Ty = axis_matrix(H, y0, ch, Ho, bool(flip & 2), mode)
        Wx, Tx = axis_matrix(W, x0, cw, Wo, bool(flip & 1), mode)
        num = np.einsum("ys,scx->ycx", Wy, np.einsum("swc,xw->scx", a.astype(np.int64), Wx)).transpose(0, 2, 1)     # [Ho, Wo, C]
        den = Ty * Tx
        assert int(Wy.sum(1).min()) == int(Wy.sum(1).max()) == Ty and int(Wx.sum(1).min()) == int(Wx.sum(1).max()) == Tx
        if out == "f32":
            res = (num.astype(np.float64) / np.float64(255 * den)).astype(np.float32)
        else:
            assert out == "u8"
            res = ((2 * num + den) // (2 * den)).astype(np.uint8)
    else:
        assert a.dtype == np.float32 and mode in (NEAREST, BILINEAR) and out == "f32"
        iy, wy, Ty = axis_taps(y0, ch, Ho, bool(flip & 2), mode)
        ix, wx, Tx = axis_taps(x0, cw, Wo, bool(flip & 1), mode)
        acc = None
        with np.errstate(invalid="ignore", over="ignore"):
            for ky in range(iy.shape[1]):                    # row-major over the taps, each add rounded once
                for kx in range(ix.shape[1]):
                    w = (wy[:, ky][:, None] * wx[:, kx][None, :]).astype(np.float64)[:, :, None]
                    term = w * a[iy[:, ky]][:, ix[:, kx]].astype(np.float64)
                    acc = term if acc is None else acc + term
            res = (acc / np.float64(Ty * Tx)).astype(np.float32)
    return res[:, :, 0] if squeeze else res


def row_ok(r, C, src_elems, dst_elems, max_dst_pixels, max_side=8192):
    """The header's row conditions, in Python integers."""
    so, sh, sw, srs, sps, scs, y0, x0, ch, cw, flip, do, dh, dw, drs, dps, dcs, rsv = (int(v) for v in r)
    return (all(1 <= v <= max_side for v in (sh, sw, ch, cw, dh, dw)) and y0 >= 0 and x0 >= 0 and y0 + ch <= sh and x0 + cw <= sw
            and min(srs, sps, scs, drs, dps, dcs) >= 1 and 0 <= flip <= 3 and rsv == 0 and so >= 0 and do >= 0
            and so + (sh - 1) * srs + (sw - 1) * sps + (C - 1) * scs < src_elems
            and do + (dh - 1) * drs + (dw - 1) * dps + (C - 1) * dcs < dst_elems and dh * dw <= max_dst_pixels)


def run_table(src, dst, table, C, mode, max_dst_pixels):
    """What camo_resize leaves in ``dst`` (a flat array, changed in place) and in status, for flat ``src`` and a [N, 18] table; rows
    in order.  A refused row with a good destination gets zeros where its stated destination lies inside dst."""
    status = []
    out = "u8" if dst.dtype == np.uint8 else "f32"
    for r in np.asarray(table).tolist():
        so, sh, sw, srs, sps, scs, y0, x0, ch, cw, flip, do, dh, dw, drs, dps, dcs, rsv = r
        yy, xx, cc = np.meshgrid(np.arange(max(dh, 0)), np.arange(max(dw, 0)), np.arange(C), indexing="ij")
        if not row_ok(r, C, src.size, dst.size, max_dst_pixels):
            status.append(1)
            if do >= 0 and 1 <= dh <= 8192 and 1 <= dw <= 8192 and min(drs, dps, dcs) >= 1 and dh * dw <= max_dst_pixels:
                at = do + yy * drs + xx * dps + cc * dcs
                dst[at[at < dst.size]] = 0
            continue
        status.append(0)
        sy, sx, sc = np.meshgrid(np.arange(sh), np.arange(sw), np.arange(C), indexing="ij")
        img = src[so + sy * srs + sx * sps + sc * scs]
        dst[do + yy * drs + xx * dps + cc * dcs] = resize(img, (dh, dw), mode, (y0, x0, ch, cw), flip, out)
    return np.array(status, np.int32)
