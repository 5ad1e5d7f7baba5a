"""The augmentation kernels (include/camo_augment.h) against tests/augment_ref.py.

PARITY UNPINNED: the header is the definition, the numpy restatement the checker.  The definition is exact integers, so every GPU
comparison is ``np.array_equal``; there is no tolerance on the kernels anywhere in this file.  The CPU tests hold the header to the
binding, the library's argument checks to the header, the restatement to tests/resize_ref.py on axis-aligned maps (equality), to
``np.rot90`` on quarter turns (equality) and to ``PIL.ImageEnhance`` one enhancement at a time (one grey level: PIL computes in
floating point; the four in sequence are NOT compared, single-level differences grow through the sharpness extrapolation).
The GPU tests run the raw call between guard bands (tests/guarded.py) on a workspace of exactly camo_augment_workspace_bytes filled
with 0xA5, and hold the inputs to being unchanged.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import augment_ref as AR
import resize_ref as RR
from conftest import ROOT
from guarded import Arrays

E_ARG = -1
ONE = 1 << 16
FILL = 0xE0A15B3C                                                       # a different byte per channel, none of them 0
SOURCES = ((1, 1), (1, 7), (5, 7), (37, 53), (64, 96))                  # 37 x 53 x 3 = 5883 bytes: the last pixel's 32-bit fetch would cross src_elems
DESTS = {(1, 1): 3, (2, 5): 17, (3, 3): 1, (33, 31): 17, (31, 33): 3, (33, 32): 17, (64, 96): 17}      # destination -> N of its batch


def axis_rows(H, W, Ho, Wo, crop=None, flip=0):
    """The axis-aligned map of the header's text for a crop and a flip: (clip = the crop, the six integers)."""
    y0, x0, ch, cw = (0, 0, H, W) if crop is None else crop
    ax, ay = int(np.rint(cw * 32768 / Wo)), int(np.rint(ch * 32768 / Ho))
    bx, by = (2 * x0 - 1) * 32768, (2 * y0 - 1) * 32768
    if flip & 1:
        ax, bx = -ax, (2 * (x0 + cw) - 1) * 32768
    if flip & 2:
        ay, by = -ay, (2 * (y0 + ch) - 1) * 32768
    return (y0, x0, ch, cw), (ax, 0, bx, 0, ay, by)


def quarter_turns(H, W):
    """(k, the six integers) with which a [H, W] image comes out as np.rot90(img, k), at the size of that."""
    h = ONE // 2
    return ((1, (0, -h, (2 * W - 1) * h, h, 0, -h)),                    # out[i, j] = img[j, W - 1 - i]
            (2, (-h, 0, (2 * W - 1) * h, 0, -h, (2 * H - 1) * h)),      # out[i, j] = img[H - 1 - i, W - 1 - j]
            (3, (0, h, -h, -h, 0, (2 * H - 1) * h)))                    # out[i, j] = img[H - 1 - j, i]


def rotation(H, W, Ho, Wo, degrees, zoom):
    """A turn about the image's centre at ``zoom``, isotropic: one source pixel a destination pixel at zoom 1."""
    t = math.radians(degrees)
    m00, m01, m10, m11 = math.cos(t) / zoom, -math.sin(t) / zoom, math.sin(t) / zoom, math.cos(t) / zoom
    b0 = (W / 2 - 0.5 - m00 * Wo / 2 - m01 * Ho / 2) * ONE
    b1 = (H / 2 - 0.5 - m10 * Wo / 2 - m11 * Ho / 2) * ONE
    return tuple(int(np.rint(v)) for v in (m00 * 32768, m01 * 32768, b0, m10 * 32768, m11 * 32768, b1))


def maps_for(H, W, Ho, Wo):
    """The maps of the GPU tests for one source and destination size."""
    h = ONE // 2
    out = [axis_rows(H, W, Ho, Wo, None, f)[1] for f in range(4)]                              # the resize, and each flip
    out += [m for _, m in quarter_turns(H, W)]
    out += [rotation(H, W, Ho, Wo, 15.0, 0.8), rotation(H, W, Ho, Wo, -15.0, 1.25)]
    out.append((h, 0, 1 << 40, 0, h, -h))                                                      # wholly outside the clip box: all fill
    out.append((0, 0, (W // 2) * ONE + 777, 0, 0, (H // 2) * ONE + 40000))                     # the zero matrix: every pixel the same source point
    out.append((h // 64, 0, (W // 3) * ONE, 0, h // 64, (H // 3) * ONE - 5))                   # a 64 x magnification
    out.append((1 << 30, -(1 << 30), -(1 << 46), -(1 << 30), 1 << 30, 1 << 46))                # the largest integers: negative floors, no overflow
    out.append((-(1 << 30), 1 << 30, 1 << 46, 1 << 30, 1 << 30, -(1 << 46)))
    out.append((h, 0, -h, 0, h, -h))                                                           # X, Y exactly on the integers
    out.append((h, 0, -h - 1, 0, h, -h - 1))                                                   # one unit below 0: a blend of the fill and pixel 0
    return out


def batch(N, C, Ho, Wo, shift=0, seed=0, factors=None):
    """(flat uint8 source, table [N, 24]): image i has source size i mod 5 and map (i + shift) of ``maps_for``; borders, clip boxes
    (whole image or a box inside it) and packed / planar layouts alternate."""
    rs = np.random.RandomState(seed)
    chunks, rows, at = [], [], 0
    for i in range(N):
        H, W = SOURCES[(i + shift) % len(SOURCES)]
        img = rs.randint(0, 256, size=(H, W, C)).astype(np.uint8)
        ms = maps_for(H, W, Ho, Wo)
        mat = ms[(i + shift) % len(ms)]
        clip = (H // 4, W // 4, H - H // 2, W - W // 2) if i % 3 == 0 else (0, 0, H, W)
        if i % 4 == 3:                                                   # planar
            chunks.append(img.transpose(2, 0, 1).reshape(-1))
            geo = [at, H, W, W, 1, H * W]
        else:
            chunks.append(img.reshape(-1))
            geo = [at, H, W, W * C, C, 1]
        k = (0, 0, 0, 0) if factors is None else factors[i % len(factors)]
        rows.append(geo + list(clip) + list(mat) + [(i // 2) % 2, FILL & ((1 << (8 * C)) - 1) if i % 5 else FILL] + list(k) + [0, 0])
        at += H * W * C
    return np.concatenate(chunks), np.array(rows, np.int64)


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_header_symbol_binding_and_constants():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_augment.h")).read()
    assert _lib.symbols("camo_augment.h") == ("camo_augment_workspace_bytes", "camo_augment")
    assert "PARITY UNPINNED" in hdr and "NOT the same" in hdr and "NOT BUILT" in hdr
    for word in ("fp32 sources", "AREA filter", "shear", "pepper noise", "C != 3"):
        assert word in hdr, word
    assert _lib.ABI_VERSION == 13 and _lib.lib().camo_abi_version() == 13
    macros = dict(re.findall(r"^#define (CAMO_AUG_\w+) (\d+)", hdr, re.M))
    assert len(macros) == 4 and AR.FIELDS == int(macros["CAMO_AUG_FIELDS"]) and AR.F == int(macros["CAMO_AUG_FRAC_BITS"])
    for name, value in macros.items():
        assert getattr(_lib, name[len("CAMO_"):]) == int(value), name


def test_argument_checks_match_the_header():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    fake = 0x1000                                    # never dereferenced: every check runs on the host before the first launch
    U8, F32, NEAR, BIL, AREA = _lib.RSZ_U8, _lib.RSZ_F32, _lib.RSZ_NEAREST, _lib.RSZ_BILINEAR, _lib.RSZ_AREA

    def call(src=fake, src_elems=100, dst=fake, dst_type=F32, table=fake, N=2, C=3, Ho=8, Wo=8, filter=BIL, enhance=0, status=fake, ws=fake,
             ws_bytes=1 << 20):
        rc = L.camo_augment(src, src_elems, dst, dst_type, table, N, C, Ho, Wo, filter, enhance, status, ws, ws_bytes, None)
        return rc, L.camo_last_error()

    need = L.camo_augment_workspace_bytes(2, 8, 8, 3, 1)
    assert need == 256 + 2 * 8 * 8 * 4 and L.camo_augment_workspace_bytes(2, 8, 8, 3, 0) == 0
    for bad in ((0, 8, 8, 3, 1), (2, 0, 8, 3, 1), (2, 8, 8193, 3, 1), (2, 8, 8, 4, 1), (2, 8, 8, 1, 1), (2, 8, 8, 3, 2), (2, 8, 8, 5, 0)):
        assert L.camo_augment_workspace_bytes(*bad) == 0, bad
    assert L.camo_augment_workspace_bytes(17, 33, 31, 3, 1) == 256 + ((17 * 33 * 31 * 4 + 255) // 256) * 256
    for kw, word in ((dict(src=None), b"src"), (dict(dst=None), b"dst"), (dict(table=None), b"table"), (dict(status=None), b"status"),
                     (dict(N=0), b"N"), (dict(N=_lib.RGD_MAX_IMAGES + 1), b"N"), (dict(C=0), b"C"), (dict(C=_lib.RSZ_MAX_CHANNELS + 1), b"C"),
                     (dict(Ho=0), b"Ho"), (dict(Ho=_lib.RSZ_MAX_SIDE + 1), b"Ho"), (dict(Wo=0), b"Wo"), (dict(Wo=_lib.RSZ_MAX_SIDE + 1), b"Wo"),
                     (dict(filter=AREA), b"filter"), (dict(filter=-1), b"filter"), (dict(dst_type=2), b"dst_type"), (dict(dst_type=-1), b"dst_type"),
                     (dict(enhance=2), b"enhance"), (dict(enhance=-1), b"enhance"), (dict(enhance=1, C=1), b"C = 3"),
                     (dict(enhance=1, C=4), b"C = 3"), (dict(src_elems=0), b"src_elems"), (dict(dst=fake + 2), b"dst"),
                     (dict(table=fake + 4), b"table"), (dict(status=fake + 2), b"status"), (dict(enhance=1, ws=None), b"ws"),
                     (dict(enhance=1, ws=fake + 128), b"ws"), (dict(enhance=1, ws_bytes=need - 1), b"camo_augment_workspace_bytes")):
        rc, msg = call(**kw)
        assert rc == E_ARG and word in msg, (kw, rc, msg)
    assert (NEAR, U8) == (0, 0)


def test_axis_aligned_maps_equal_the_resize_reference():
    """300 random crops and flips: replicate border at the crop's edge, power-of-two destinations, so cw 2^15 / Wo is an integer."""
    rs = np.random.RandomState(0)
    for case in range(300):
        H, W, C = int(rs.randint(1, 50)), int(rs.randint(1, 50)), (1, 3)[case % 2]
        Ho, Wo = (1 << int(rs.randint(0, 7)), 1 << int(rs.randint(0, 7)))
        ch, cw = int(rs.randint(1, H + 1)), int(rs.randint(1, W + 1))
        crop = (int(rs.randint(0, H - ch + 1)), int(rs.randint(0, W - cw + 1)), ch, cw)
        flip = case % 4
        img = rs.randint(0, 256, size=(H, W, C)).astype(np.uint8)
        clip, mat = axis_rows(H, W, Ho, Wo, crop, flip)
        for out in ("u8", "f32"):
            assert np.array_equal(AR.warp(img, (Ho, Wo), clip, mat, 1, FILL, "bilinear", out), RR.resize(img, (Ho, Wo), "bilinear", crop, flip, out)), case
        assert np.array_equal(AR.warp(img, (Ho, Wo), clip, mat, 1, FILL, "nearest", "u8"), RR.resize(img, (Ho, Wo), "nearest", crop, flip, "u8")), case


def test_quarter_turns_are_rot90_and_read_no_fill():
    img = np.random.RandomState(1).randint(1, 255, size=(5, 7, 3)).astype(np.uint8)        # no byte of the image is the fill's 0xFF
    for k, mat in quarter_turns(5, 7):
        want = np.rot90(img, k)
        for mode in ("bilinear", "nearest"):
            got = AR.warp(img, want.shape[:2], (0, 0, 5, 7), mat, 0, 0xFFFFFFFF, mode, "u8")
            assert np.array_equal(got, want) and not (got == 255).any(), (k, mode)


def test_all_factors_256_is_the_identity():
    rs = np.random.RandomState(2)
    for size in ((1, 1), (2, 5), (3, 3), (17, 9)):
        img = rs.randint(0, 256, size=size + (3,)).astype(np.uint8)
        assert np.array_equal(AR.enhance(img, (256, 256, 256, 256)), img)
        for f in (AR.brightness, AR.contrast, AR.colour, AR.sharpness):
            assert np.array_equal(f(img, 256), img)
    thin = rs.randint(0, 256, size=(2, 9, 3)).astype(np.uint8)                               # a side below 3: sharpness changes nothing
    assert np.array_equal(AR.sharpness(thin, 1024), thin) and np.array_equal(AR.sharpness(thin, 0), thin)


def test_each_enhancement_is_within_a_grey_level_of_pil():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    rs = np.random.RandomState(3)
    ops = ((AR.brightness, ImageEnhance.Brightness, 128, 384), (AR.contrast, ImageEnhance.Contrast, 128, 384),
           (AR.colour, ImageEnhance.Color, 0, 512), (AR.sharpness, ImageEnhance.Sharpness, 0, 768))
    worst = [0, 0, 0, 0]
    for case in range(200):
        img = rs.randint(0, 256, size=(int(rs.randint(3, 40)), int(rs.randint(3, 40)), 3)).astype(np.uint8)
        for j, (mine, theirs, lo, hi) in enumerate(ops):
            k = int(rs.randint(lo, hi + 1))
            pil = np.asarray(theirs(Image.fromarray(img)).enhance(k / 256.0))
            worst[j] = max(worst[j], int(np.abs(mine(img, k).astype(np.int64) - pil.astype(np.int64)).max()))
    print("largest difference from PIL per enhancement (grey levels):", worst)
    assert max(worst) <= 1, worst


def test_affine_rows_gives_the_axis_aligned_integers_at_angle_zero():
    from camouflage_multimodal_amd.augment import affine_rows
    rs = np.random.RandomState(4)
    sizes, crops, flips = [], [], []
    for i in range(40):
        H, W = int(rs.randint(1, 300)), int(rs.randint(1, 300))
        ch, cw = int(rs.randint(1, H + 1)), int(rs.randint(1, W + 1))
        sizes.append((H, W))
        crops.append((int(rs.randint(0, H - ch + 1)), int(rs.randint(0, W - cw + 1)), ch, cw))
        flips.append(i % 4)
    for size in ((64, 64), (256, 128), (1, 2)):
        rep = affine_rows(sizes, size, crops, flips, border="replicate", fill=7)
        con = affine_rows(sizes, size, crops, flips, angles=[0.0] * 40, zooms=[1.0] * 40, border="constant", fill=(1, 2, 3))
        for (H, W), crop, flip, a, b in zip(sizes, crops, flips, rep, con):
            clip, mat = axis_rows(H, W, size[0], size[1], crop, flip)
            assert tuple(a) == clip + mat + (1, 0x07070707) and tuple(b) == (0, 0, H, W) + mat + (0, 0x030201)
    # a half turn is both flips; a zoom of 2 halves the matrix and keeps the centre
    (r,), (f,) = affine_rows([(30, 50)], (64, 64), angles=[180.0]), affine_rows([(30, 50)], (64, 64), flips=[3])
    assert max(abs(a - b) for a, b in zip(r, f)) <= 1
    (z,), (p,) = affine_rows([(32, 64)], (64, 64), zooms=[2.0]), affine_rows([(32, 64)], (64, 64))
    assert z[4:6] == [p[4] // 2, 0] and z[7:9] == [0, p[8] // 2] and z[4] * 64 + z[6] == p[4] * 64 + p[6]       # the centre's X: a00 Wo + b0
    for kw in (dict(border="reflect"), dict(crops=[(0, 0, 31, 50)]), dict(flips=[4]), dict(zooms=[0.0]), dict(angles=[float("nan")]),
               dict(fill=256), dict(fill=(1, 2, 3, 4, 5)), dict(angles=[0.0, 1.0])):
        with pytest.raises(ValueError):
            affine_rows([(30, 50)], (64, 64), **kw)
    with pytest.raises(ValueError, match="size"):
        affine_rows([(30, 50)], (0, 64))


def test_random_cod_augmentation_is_reproducible_and_in_range():
    from camouflage_multimodal_amd.augment import affine_rows, random_cod_augmentation
    sizes = [(40 + 7 * i, 30 + (13 * i) % 70) for i in range(50)]
    a, b, c = random_cod_augmentation(sizes, seed=5), random_cod_augmentation(sizes, seed=5), random_cod_augmentation(sizes, seed=6)
    assert a == b and a != c and set(a) == {"crops", "flips", "angles", "factors"}
    assert all(len(a[k]) == 50 for k in a)
    for (H, W), (y0, x0, h, w), f, ang, ks in zip(sizes, a["crops"], a["flips"], a["angles"], a["factors"]):
        assert 0 <= y0 and 0 <= x0 and 1 <= h and 1 <= w and y0 + h <= H and x0 + w <= W and f in (0, 1) and -15.0 <= ang <= 15.0
        assert 128 <= ks[0] <= 384 and 128 <= ks[1] <= 384 and 0 <= ks[2] <= 512 and 0 <= ks[3] <= 768 and all(isinstance(k, int) for k in ks)
    turned = sum(1 for ang in a["angles"] if ang != 0.0)
    assert 0 < turned < 50                                                # rotate_p = 0.2
    assert all(ang == 0.0 for ang in random_cod_augmentation(sizes, seed=5, rotate_p=0.0)["angles"])
    none = random_cod_augmentation(sizes, seed=5, brightness=None, contrast=None, colour=None, sharpness=None)
    assert none["factors"] is None and len(none["crops"]) == 50
    one = random_cod_augmentation(sizes, seed=5, contrast=None, sharpness=None, colour=(9.0, 9.0))
    assert all(k[1] == 256 and k[3] == 256 and k[2] == 1024 for k in one["factors"])       # a range past 4 stops at 1024
    rows = affine_rows(sizes, (64, 64), a["crops"], a["flips"], a["angles"])
    assert all(AR.row_ok([0, H, W, 3 * W, 3, 1] + r + list(k) + [0, 0], 3, H * W * 3, True) for (H, W), r, k in zip(sizes, rows, a["factors"]))


def test_random_cod_augmentation_pinned_draws():
    """The order and number of draws from the generator are part of the function: a seed gives exactly this dict."""
    from camouflage_multimodal_amd.augment import random_cod_augmentation
    assert random_cod_augmentation([(33, 70), (8, 9), (600, 800)], seed=5) == {
        "crops": [(0, 8, 33, 42), (1, 1, 7, 6), (2, 4, 591, 769)], "flips": [1, 0, 0], "angles": [0.0, 0.0, 0.0],
        "factors": [(253, 382, 414, 499), (132, 152, 423, 640), (344, 286, 288, 283)]}


GOOD = [0, 8, 9, 27, 3, 1, 1, 2, 6, 5, 32768, 0, -32768, 0, 32768, -32768, 0, FILL, 256, 0, 1024, 300, 0, 0]
# one row per violated condition: (field, value, only with enhance = 1)
VIOLATIONS = ((1, 0, False), (1, 8193, False), (2, 0, False), (8, 0, False), (9, 8193, False), (6, -1, False), (7, -1, False), (6, 3, False),
              (7, 5, False), (3, 0, False), (4, 0, False), (5, 0, False), (0, -1, False), (0, 1, False), (3, 1 << 62, False), (4, 1 << 62, False),
              (10, (1 << 30) + 1, False), (11, -(1 << 30) - 1, False), (13, (1 << 30) + 1, False), (14, -(1 << 30) - 1, False),
              (12, (1 << 46) + 1, False), (15, -(1 << 46) - 1, False), (16, 2, False), (16, -1, False), (17, -1, False), (17, 1 << 32, False),
              (22, 1, False), (23, -1, False), (18, 1025, True), (19, -1, True), (20, 1025, True), (21, -1, True))


def test_row_validity_by_hand():
    from camouflage_multimodal_amd.augment import check_rows
    elems = 8 * 9 * 3
    for enh in (False, True):
        assert AR.row_ok(GOOD, 3, elems, enh)
        check_rows([GOOD], 3, elems, enh)
        assert not AR.row_ok(GOOD, 3, elems - 1, enh) and not AR.row_ok(GOOD, 4, elems, enh)
        for field, value, enh_only in VIOLATIONS:
            bad = list(GOOD)
            bad[field] = value
            assert AR.row_ok(bad, 3, elems, enh) == (enh_only and not enh), (field, value, enh)
            if enh or not enh_only:
                with pytest.raises(ValueError, match="image 0"):
                    check_rows([bad], 3, elems, enh)
    edge = list(GOOD)                                                     # the bounds themselves are good
    edge[10], edge[14], edge[12], edge[15], edge[17], edge[18] = 1 << 30, -(1 << 30), 1 << 46, -(1 << 46), (1 << 32) - 1, 1024
    assert AR.row_ok(edge, 3, elems, True)


def test_cpu_tensors_and_bad_arguments_raise():
    from camouflage_multimodal_amd import RaggedImages, prepare_finetune_batch_ragged
    from camouflage_multimodal_amd._lib import CamoError
    from camouflage_multimodal_amd.augment import augment_batch, augment_table, random_cod_augmentation
    t = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(CamoError):
        augment_batch(t, (4, 4))
    with pytest.raises(CamoError):
        augment_batch(RaggedImages(torch.zeros(8 * 9 * 3, dtype=torch.uint8), [(8, 9)], 3), (4, 4))
    with pytest.raises(CamoError):
        augment_table(torch.zeros(8 * 9 * 3, dtype=torch.uint8), [GOOD], 3, (4, 4))
    with pytest.raises(ValueError, match="out_dtype"):                   # (before anything touches a device)
        augment_batch(t, (4, 4), out_dtype=torch.float16)
    with pytest.raises(ValueError, match="filter"):
        augment_batch(t, (4, 4), filter="area")
    with pytest.raises(ValueError, match="size"):
        augment_batch(t, (0, 4))
    with pytest.raises(ValueError, match="size"):
        augment_table(t, [GOOD], 3, (4, 8193))
    with pytest.raises(ValueError, match="3 channels"):
        augment_table(t, [GOOD], 1, (4, 4), enhance=True)
    img, mask = np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9), np.uint8)
    aug = random_cod_augmentation([(8, 9)], seed=0)
    with pytest.raises(ValueError, match="crops and flips"):
        prepare_finetune_batch_ragged([img], [mask], crops=[(0, 0, 8, 9)], augment=aug, device="cpu")
    with pytest.raises(ValueError, match="crops and flips"):
        prepare_finetune_batch_ragged([img], [mask], flips=[0], augment=aug, device="cpu")
    with pytest.raises(CamoError):
        prepare_finetune_batch_ragged([img], [mask], augment=aug, device="cpu")


# ---- GPU ------------------------------------------------------------------------------------------------------------------

class Call:
    """The raw camo_augment between guard bands: every array in a guarded tensor of its own, dst and status filled with patterns the
    call must overwrite, the workspace exactly camo_augment_workspace_bytes and 0xA5."""

    def __init__(self, src, table, C, size, mode, enhance, out):
        from camouflage_multimodal_amd import _lib
        self.L, self._lib = _lib.lib(), _lib
        self.N, self.C, self.size, self.mode, self.enhance, self.out = len(table), C, size, mode, int(enhance), out
        self.need = int(self.L.camo_augment_workspace_bytes(self.N, size[0], size[1], C, self.enhance))
        assert (self.need > 0) == bool(enhance)
        self.A = Arrays({"src": ((src.size,), np.uint8), "table": ((self.N, AR.FIELDS), np.int64),
                         "dst": ((self.N, size[0], size[1], C), np.uint8 if out == "u8" else np.float32), "status": ((self.N,), np.int32),
                         "ws": self.need}, {None: 0xA5, "status": 0x7F, "src": 0x00, "table": 0x00}, {None: 0, "src": 1})
        self.put(src, table)

    def put(self, src, table):
        self.src, self.table = src.copy(), table.copy()
        self.A.piece["src"].copy_(torch.from_numpy(self.src))
        self.A.piece["table"].copy_(torch.from_numpy(self.table.view(np.uint8).reshape(-1)))

    def run(self):
        A, lib = self.A, self._lib
        rc = self.L.camo_augment(A.ptr("src"), self.src.size, A.ptr("dst"), lib.RSZ_U8 if self.out == "u8" else lib.RSZ_F32, A.ptr("table"), self.N,
                                 self.C, self.size[0], self.size[1], {"nearest": lib.RSZ_NEAREST, "bilinear": lib.RSZ_BILINEAR}[self.mode],
                                 self.enhance, A.ptr("status"), A.ptr("ws"), self.need, None)
        assert rc == 0, self.L.camo_last_error()
        got = A.collect()                                                 # (synchronises and checks every guard)
        assert np.array_equal(got["src"], self.src) and np.array_equal(got["table"], self.table), "an input was written"
        return got["dst"], got["status"]

    def check(self, note=""):
        dst, status = self.run()
        want, wstatus = AR.run_table(self.src, self.table, self.C, self.size, self.mode, self.enhance, self.out)
        assert np.array_equal(status, wstatus), (note, status, wstatus)
        for i in range(self.N):
            assert np.array_equal(dst[i], want[i]), (note, "image", i, self.table[i].tolist())
        return dst


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_warp_equals_the_reference(mode, out, C):
    for j, (size, N) in enumerate(DESTS.items()):
        for shift in ((j, j + 7) if N < 17 else (j,)):
            src, table = batch(N, C, size[0], size[1], shift=shift + C, seed=100 + j)
            dst = Call(src, table, C, size, mode, 0, out).check((mode, out, C, size))
            assert dst.shape == (N,) + size + (C,)


@pytest.mark.gpu
@pytest.mark.parametrize("out", ["u8", "f32"])
def test_every_map_on_the_source_whose_last_fetch_crosses_the_buffer(out):
    """37 x 53 x 3 alone in its buffer, every map with both borders, two blocks per image; fields 18 .. 21 are not read with
    enhance = 0, whatever they hold."""
    H, W, size = 37, 53, (33, 32)
    img = np.random.RandomState(7).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    rows = [[0, H, W, 3 * W, 3, 1, 0, 0, H, W] + list(m) + [border, FILL, 5000, -1, 1 << 40, 7, 0, 0] for m in maps_for(H, W, *size) for border in (0, 1)]
    for mode in ("bilinear", "nearest"):
        Call(img.reshape(-1), np.array(rows, np.int64), 3, size, mode, 0, out).check((mode, out))


FACTOR_SETS = tuple((256,) * j + (k,) + (256,) * (3 - j) for j in range(4) for k in (0, 256, 1024, 141)) + ((90, 400, 30, 900),)


@pytest.mark.gpu
@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_enhancements_equal_the_reference(mode, out):
    """Each factor alone at 0, 256, 1024 and a value between, and the four together, on every destination size; the second call of
    each pair runs on the workspace the first one left, with other images: a luma sum that is not cleared would show."""
    assert len(FACTOR_SETS) == 17
    for j, size in enumerate(DESTS):
        src, table = batch(17, 3, size[0], size[1], shift=j, seed=200 + j, factors=FACTOR_SETS)
        call = Call(src, table, 3, size, mode, 1, out)
        call.check((mode, out, size))
        src2, table2 = batch(17, 3, size[0], size[1], shift=j, seed=300 + j, factors=FACTOR_SETS[::-1])
        assert src2.size == src.size
        call.put(255 - src2, table2)
        call.check((mode, out, size, "second call"))


@pytest.mark.gpu
def test_enhancements_on_flat_and_noise_images():
    rs = np.random.RandomState(8)
    H, W = 20, 24
    imgs = [np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)]
    ident = axis_rows(H, W, H, W)[1]
    rows = [[i * H * W * 3, H, W, 3 * W, 3, 1, 0, 0, H, W] + list(ident) + [0, 0] + list(k) + [0, 0]
            for k in ((0, 0, 0, 0), (1024, 1024, 1024, 1024), (256, 256, 256, 256), (90, 400, 30, 900)) for i in range(3)]
    src = np.concatenate([im.reshape(-1) for im in imgs])
    dst = Call(src, np.array(rows, np.int64), 3, (H, W), "bilinear", 1, "u8").check()
    assert np.array_equal(dst[6], imgs[0]) and np.array_equal(dst[7], imgs[1]) and np.array_equal(dst[8], imgs[2])     # all 256: the identity
    assert (dst[3] == 0).all() and (dst[4] == 255).all()                 # a flat image has nothing to enhance
    f32 = Call(src, np.array(rows, np.int64), 3, (H, W), "bilinear", 1, "f32").check()
    assert np.array_equal(f32[8], (imgs[2].astype(np.float64) / 255.0).astype(np.float32))


@pytest.mark.gpu
def test_repeatable_and_batch_equals_single_images():
    from camouflage_multimodal_amd import pack_images
    from camouflage_multimodal_amd.augment import affine_rows, augment_batch
    rs = np.random.RandomState(9)
    images = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SOURCES]
    packed = pack_images(images)
    rows = affine_rows(SOURCES, (33, 32), angles=[0.0, 15.0, -15.0, 7.5, 90.0], zooms=[1.0, 0.8, 1.25, 1.0, 2.0], flips=[0, 1, 2, 3, 0], fill=(9, 8, 7))
    ks = FACTOR_SETS[12:]
    for factors in (None, ks):
        for dtype in (torch.uint8, torch.float32):
            a = augment_batch(packed, (33, 32), rows, factors, out_dtype=dtype)
            b = augment_batch(packed, (33, 32), rows, factors, out_dtype=dtype)
            assert a.dtype == dtype and tuple(a.shape) == (5, 33, 32, 3) and torch.equal(a, b)
            for i, im in enumerate(images):                               # N = 1, five times
                one = augment_batch([im], (33, 32), [rows[i]], None if factors is None else [ks[i]], out_dtype=dtype)
                assert torch.equal(one[0], a[i]), (i, dtype)
            want = [AR.warp(im, (33, 32), r[:4], r[4:10], r[10], r[11], "bilinear", "u8") for im, r in zip(images, rows)]
            if factors is not None:
                want = [AR.enhance(w, k) for w, k in zip(want, ks)]
            if dtype == torch.uint8:
                assert np.array_equal(a.cpu().numpy(), np.stack(want))
    grey = [im[:, :, 0].copy() for im in images]                         # [H, W] images come back [N, Ho, Wo]
    g = augment_batch(grey, (33, 32), [r[:11] + [9] for r in rows], filter="nearest", out_dtype=torch.uint8)
    assert tuple(g.shape) == (5, 33, 32)
    assert np.array_equal(g.cpu().numpy(), np.stack([AR.warp(im, (33, 32), r[:4], r[4:10], r[10], 9, "nearest", "u8") for im, r in zip(grey, rows)]))


@pytest.mark.gpu
@pytest.mark.parametrize("enhance", [0, 1])
def test_the_kernel_refuses_a_bad_row_and_touches_nothing_outside(enhance):
    """A device table is not checked on the host.  One row per violated condition between two good neighbours in one packed buffer:
    status 1 and zeros for it, the neighbours as the reference has them, every guard whole."""
    rs = np.random.RandomState(10)
    elems, size = 8 * 9 * 3, (33, 32)
    src = rs.randint(0, 256, size=3 * elems).astype(np.uint8)
    left, right = list(GOOD), list(GOOD)
    left[0], right[0] = 0, 2 * elems
    right[10:16] = rotation(8, 9, 33, 32, 15.0, 0.3)
    for field, value, enh_only in VIOLATIONS:
        bad = list(GOOD)
        bad[0] = elems
        bad[field] = value if field != 0 else (-1 if value < 0 else 3 * elems - 8 * 9 * 3 + 1)        # (an offset that leaves the buffer by one byte)
        call = Call(src, np.array([left, bad, right], np.int64), 3, size, "bilinear", enhance, "f32" if field % 2 else "u8")
        dst = call.check((field, value))
        refused = not enh_only or enhance == 1
        _, status = AR.run_table(src, call.table, 3, size, "bilinear", enhance, "u8")
        assert status.tolist() == [0, 1 if refused else 0, 0], (field, value)
        assert (dst[1] == 0).all() == refused and (dst[0] != 0).any() and (dst[2] != 0).any(), (field, value)


@pytest.mark.gpu
def test_bad_arguments_raise_by_name_on_the_host():
    from camouflage_multimodal_amd.augment import affine_rows, augment_batch, augment_table
    t = torch.zeros(2, 8, 9, 3, dtype=torch.uint8, device="cuda")
    rows = affine_rows([(8, 9)] * 2, (4, 4))
    assert tuple(augment_batch(t, (4, 4), rows).shape) == (2, 4, 4, 3)
    for kw, word in ((dict(rows=rows[:1]), "rows"), (dict(rows=[r[:11] for r in rows]), "rows"), (dict(factors=[(256,) * 4]), "factors"),
                     (dict(factors=[(256,) * 3] * 2), "factors"), (dict(factors=[(256, 256, 256, 1025)] * 2), "factor"),
                     (dict(factors=[(-1, 256, 256, 256)] * 2), "factor"), (dict(rows=[rows[0], rows[1][:4] + [1 << 31] + rows[1][5:]]), "map"),
                     (dict(rows=[rows[0], [0, 0, 9, 9] + rows[1][4:]]), "clip box"), (dict(rows=[rows[0], rows[1][:10] + [2, 0]]), "border"),
                     (dict(filter="area"), "filter"), (dict(out_dtype=torch.int32), "out_dtype"), (dict(size=(4, 9000)), "size")):
        with pytest.raises(ValueError, match=word):
            augment_batch(t, **{"size": (4, 4), "rows": rows, **kw})
    with pytest.raises(ValueError, match="3 channels"):
        augment_batch(t[..., 0].contiguous(), (4, 4), rows, [(256,) * 4] * 2)
    with pytest.raises(ValueError, match="uint8"):
        augment_table(t.float(), [GOOD], 3, (4, 4))
    with pytest.raises(ValueError, match="table"):
        augment_table(t, [GOOD[:23]], 3, (4, 4))
    with pytest.raises(ValueError, match="footprint"):
        augment_table(t, [GOOD], 3, (4, 4), src_elems=8 * 9 * 3 - 1)
