"""The benchmark-measure kernels (csrc/seg_measures.hip) at the sizes where their code takes another path than at the
33 x 70 and 130 x 257 of test_seg_measures.py and test_seg_weighted_f.py.  The checker is tests/seg_measures_ref.py, unchanged, and the
checks are those files' own (`_check_tables`: hist and split integer for integer, pixels per image, two calls, a contiguous copy, a
batch the rows of its images; `_check`: n_fg exact, A_fg and A_bg within H * W units of 2^-32, F-beta-w within 1e-6).

Every size below is computed from the kernels' constants (csrc/seg_measures.h, read by regex; SEG_WF_MAX_SIDE from the binding), so
a retuned constant moves the case with it.  With today's constants:

  fill kernel, second trip of the grid-stride loop   1024 x 1030 (a = 0; 65920 spans = 256 blocks x 256 lanes + 384: the second trip
                                                     has a full block, a half block and 254 blocks without work) and 1025 x 1029,
                                                     1025 x 1030, 1025 x 1031 (H * W = 1, 2, 3 mod 4 as channel 1 of [1, 3, H, W]: span 0
                                                     starts 1, 2, 3 floats before the image)
  fill kernel, SEGM_UNIFORM_LANES                    32 x 64, the first k = 7, 8, 9, 64 spans constant: k lanes of wave 0 flush one key in
                                                     step 15 beside 64 - k lanes that flush others
  both histogram kernels, no aligned chunk / W < 4   1 x 2, 2 x 1, 1 x 3, 3 x 5, 4 x 4, 1 x 17, 17 x 2, 70 x 1, 1 x 70, 3 x 341 in batches of 5
  weighted F, x += SEGM_NT and a second column block 9 x 300, 300 x 3, 40 x 257
  weighted F, the longest distance                   1 x 2048 and 2048 x 1, the one positive pixel at the far end
  weighted F, the tie rule's two halves              6 x 6 diagonal (smaller y' against the scan order), 7 x 5 column (the column pass)

Each input has a CPU test that shows, from the restatement and the constants alone, that it has the property it is named for.
"""
import functools
import math
import os
import re
import time

import numpy as np
import pytest
import torch

import seg_measures_ref as R
import test_seg_measures as T
import test_seg_weighted_f as WF
from conftest import ROOT

_NAMES = ("SEGM_NT", "SEGM_SPAN", "SEGM_SPANS_PER_LANE", "SEGM_MAX_BLOCKS", "SEGM_UNIFORM_LANES", "SEGM_WF_TILE_X", "SEGM_WF_TILE_Y")


def _header_constants():
    text = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "seg_measures.h")).read()
    return {n: int(re.search(rf"constexpr int {n} = (\d+);", text).group(1)) for n in _NAMES}


NT, SPAN, PER_LANE, MAX_BLOCKS, UNIFORM, TILE_X, TILE_Y = (_header_constants()[n] for n in _NAMES)
GRID_SPANS = MAX_BLOCKS * NT                                   # spans the largest grid takes in one trip of the fill kernel's loop


def _max_side():
    from camouflage_multimodal_amd import _lib
    return _lib.SEG_WF_MAX_SIDE


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _nspans(HW, a):
    """The fill kernel's span count of an image whose first float lies a floats past a 16-byte boundary."""
    return (HW + a + SPAN - 1) // SPAN


def test_the_cases_can_be_built_from_the_constants():
    assert NT % 64 == 0 and SPAN % 4 == 0 and PER_LANE >= 1 and MAX_BLOCKS >= 2
    assert 2 <= UNIFORM - 1 and UNIFORM + 1 < 64                     # k = UNIFORM - 1, UNIFORM, UNIFORM + 1 and 64 are four different cases
    assert TILE_X * TILE_Y == NT and NT + 44 <= _max_side()


# ---- 1. the histograms past the block cap ----------------------------------------------------------------------------------------

BIG_KINDS = ("uniform", "painted", "mod1", "mod2", "mod3")


def _big_shape(kind):
    """uniform, painted: H * W a multiple of 4 (a = 0), one and a half blocks of spans past the grid.  mod r: H odd and H * W = r mod 4,
    so channel 1 of a [1, 3, H, W] tensor starts r floats past a 16-byte boundary; at least one block of spans past the grid."""
    side = math.isqrt(GRID_SPANS * SPAN)
    if not kind.startswith("mod"):
        H = side - side % 4
        return H, -(-(GRID_SPANS + 3 * NT // 2) * SPAN // H)
    H, r = side | 1, int(kind[3:])
    W = -(-(GRID_SPANS + NT) * SPAN // H) + 1
    while H * W % 4 != r:
        W += 1
    return H, W


@functools.lru_cache(maxsize=None)
def _big_case(kind):
    """(pred [1, H, W], gt [1, H, W], hist, split) of one image past SEGM_MAX_BLOCKS blocks.  Never written to."""
    H, W = _big_shape(kind)
    seed = 40 + BIG_KINDS.index(kind)
    gt = T._blobs(H, W, seed, k=4)
    yy, xx = np.mgrid[:H, :W]
    for cy, cx, r, v in ((H // 3, W // 4, H // 5, 255), (H - H // 6, W - W // 5, H // 4, 200), (H // 2, W - 1, H // 7, 128)):
        gt[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = v
    pred = T._painted(H, W, seed, 12) if kind == "painted" else T._uniform(H, W, seed)
    hist, split = R.table(pred[None], gt[None])
    return _freeze(pred[None], gt[None], hist, split)


def test_the_large_images_take_a_second_trip_with_a_ragged_end():
    if (NT, SPAN, MAX_BLOCKS) == (256, 16, 256):                     # today's constants: the sizes the docstring and DESIGN.md 10f quote
        assert _big_shape("uniform") == _big_shape("painted") == (1024, 1030)
        assert [_big_shape(f"mod{r}") for r in (1, 2, 3)] == [(1025, 1029), (1025, 1030), (1025, 1031)]
    for kind in BIG_KINDS:
        H, W = _big_shape(kind)
        a = H * W % 4                                                # channel 1 of [1, 3, H, W] on a 16-byte aligned base starts H * W floats in
        assert a == (int(kind[3:]) if kind.startswith("mod") else 0), kind
        n = _nspans(H * W, a)
        host = (H * W + 3 + SPAN - 1) // SPAN                        # the launcher's bound on the spans, which sizes the grid
        assert min(-(-host // (NT * PER_LANE)), MAX_BLOCKS) == MAX_BLOCKS
        assert -(-n // GRID_SPANS) == 2 and 0 < n % GRID_SPANS < GRID_SPANS // 2, (kind, n)
        # the second trip: blocks with all their lanes at work, a block that is cut (span >= nspans in some lanes), blocks with none
        rest = n - GRID_SPANS
        assert rest >= NT and rest % NT != 0 and -(-rest // NT) < MAX_BLOCKS, (kind, rest)
    pred, gt, hist, split = _big_case("uniform")
    H, W = pred.shape[1:]
    assert hist.sum() == H * W and hist[0, :, 1].sum() == (gt > 127).sum() > H * W // 10
    assert (hist[0].reshape(4, -1).sum(1) > 0).all()                 # pixels in every quadrant
    q, flat = R.quantise(pred[0]).ravel(), (gt[0] > 127).ravel()
    tail = slice(GRID_SPANS * SPAN, None)                            # the pixels of the second trip: both classes, many bins
    assert flat[tail].any() and (~flat[tail]).any() and len(np.unique(q[tail])) == 256
    assert np.isnan(pred[0, 0, 0]) and np.isinf(pred[0, 0, 3]) and np.isinf(pred[0, 0, 4])


def test_the_painted_large_image_is_piecewise_constant():
    pred = _big_case("painted")[0][0]
    q = R.quantise(pred)
    assert len(np.unique(q)) <= 13 and (q == 0).any() and (q == 255).any()
    runs = 1 + int((q.ravel()[1:] != q.ravel()[:-1]).sum())          # equal consecutive keys are combined: far fewer runs than pixels
    assert runs < q.size // 100


@pytest.mark.gpu
@pytest.mark.parametrize("kind", BIG_KINDS)
def test_histograms_past_the_block_cap(kind):
    pred, gt, hist, split = _big_case(kind)
    T._check_tables(pred, gt, hist, split)


# ---- 2. the uniform-lane threshold -------------------------------------------------------------------------------------------------

LANE_COUNTS = (UNIFORM - 1, UNIFORM, UNIFORM + 1, 64)
Q_CONST = 51                                                        # rintf(0.2f * 255.0f)


def _lanes_case(k):
    """H x W = 2 waves of spans, W a multiple of SEGM_SPAN.  The first k spans hold 0.2; every other pixel differs in q from the pixel
    before and after it and is never 51, and the 64 keys of wave 0 in one step are spread over 25 values.  gt: the last pixel only."""
    W = 4 * SPAN
    H = 2 * 64 * SPAN // W
    pred = ((52 + (np.arange(H * W) * 37) % 200).astype(np.float32) / np.float32(255))
    pred[: k * SPAN] = np.float32(0.2)
    gt = np.zeros((H, W), np.uint8)
    gt[H - 1, W - 1] = 255
    return pred.reshape(1, H, W), gt[None]


def _flush_pattern(pred, gt):
    """Wave 0 of block 0 of the fill kernel on one aligned image, restated from the keys: per step j the lanes that flush, the
    leader's key, how many flushing lanes share it and the count each of those holds."""
    H, W = pred.shape
    X, Y = R.split_point(gt)
    yy, xx = np.mgrid[:H, :W]
    key = (((yy >= Y) * 2 + (xx >= X)) * 512 + R.positive(gt) * 256 + R.quantise(pred)).ravel()[: 64 * SPAN].reshape(64, SPAN)
    steps, cnt = [], np.ones(64, np.int64)
    for j in range(SPAN):
        last = np.ones(64, bool) if j == SPAN - 1 else key[:, j + 1] != key[:, j]
        lanes = np.nonzero(last)[0]
        if len(lanes):
            same = lanes[key[lanes, j] == key[lanes[0], j]]
            steps.append((j, len(lanes), int(key[lanes[0], j]), len(same), cnt[same].tolist()))
        else:
            steps.append((j, 0, None, 0, []))
        cnt = np.where(last, 1, cnt + 1)
    return steps


@pytest.mark.parametrize("k", LANE_COUNTS)
def test_the_lane_cases_flush_k_lanes_of_one_key_in_the_last_step(k):
    pred, gt = _lanes_case(k)
    H, W = pred.shape[1:]
    assert W % SPAN == 0 and H * W >= 2 * 64 * SPAN and H * W % 4 == 0 and R.split_point(gt[0]) == (W, H)
    q = R.quantise(pred[0]).ravel()
    assert (q[: k * SPAN] == Q_CONST).all() and (q[k * SPAN:] != Q_CONST).all()
    rest = q[k * SPAN - 1:] if k else q
    assert (rest[1:] != rest[:-1]).all()
    steps = _flush_pattern(pred[0], gt[0])
    for j, flushing, leader, same, counts in steps[:-1]:
        assert flushing == 64 - k and same < UNIFORM, (j, flushing, same)
        assert flushing == 0 or (leader != Q_CONST and counts == [1] * same)
    j, flushing, leader, same, counts = steps[-1]
    assert (j, flushing, leader, same) == (SPAN - 1, 64, Q_CONST, k) and counts == [SPAN] * k
    assert (same >= UNIFORM) == (k >= UNIFORM)                       # k = UNIFORM - 1 adds lane by lane, the others by shuffle
    hist, _ = R.table(pred, gt)
    assert hist[0, 0, 0, Q_CONST] == SPAN * k and hist[0, 1:].sum() == 0 and hist[0, 0, 1].sum() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", LANE_COUNTS)
def test_histograms_at_the_uniform_lane_threshold(k):
    from camouflage_multimodal_amd import segmentation_histograms
    pred, gt = _lanes_case(k)
    hist, split = R.table(pred, gt)
    pt = torch.from_numpy(pred.copy()).cuda()
    assert pt.is_contiguous() and pt.data_ptr() % 16 == 0
    h, s = segmentation_histograms(pt, torch.from_numpy(gt.copy()).cuda())
    hn = h.cpu().numpy()
    print(f"k = {k}: bin {Q_CONST} holds {hn[0, 0, 0, Q_CONST]} (want {SPAN * k}), differing bins {int((hn != hist).sum())}")
    assert np.array_equal(s.cpu().numpy(), split) and np.array_equal(hn, hist)
    assert hn[0, 0, 0, Q_CONST] == SPAN * k
    T._check_tables(pred, gt, hist, split)                            # (channel 1 of [1, 3, H, W]: H * W floats in, still 16-byte aligned)


# ---- 3. tiny and thin images ------------------------------------------------------------------------------------------------------

THIN_SHAPES = ((1, 2), (2, 1), (1, 3), (3, 5), (4, 4), (1, 17), (17, 2), (70, 1), (1, 70), (3, 341))


@functools.lru_cache(maxsize=None)
def _thin_batch(shape):
    """Five images: predictions uniform in [-0.1, 1.1], random ground truths with an empty one (image 1) and a full one (image 3)."""
    H, W = shape
    rs = np.random.RandomState(1000 * H + W)
    pred = rs.uniform(-0.1, 1.1, (5, H, W)).astype(np.float32)
    gt = ((rs.uniform(size=(5, H, W)) < rs.uniform(0.2, 0.8, (5, 1, 1))) * rs.choice([128, 200, 255], (5, H, W))).astype(np.uint8)
    gt[gt == 0] = rs.choice(np.array([0, 127], np.uint8), int((gt == 0).sum()))
    gt[1], gt[3] = 0, 255
    hist, split = R.table(pred, gt)
    return _freeze(pred, gt, hist, split)


def test_the_thin_batches_hold_what_their_names_say():
    from camouflage_multimodal_amd import cod_measures
    pa, ga, worst = set(), set(), 0.0
    for H, W in THIN_SHAPES:
        pred, gt, hist, split = _thin_batch((H, W))
        assert pred.shape == (5, H, W) and not (gt[1] > 127).any() and (gt[3] > 127).all()
        assert hist.reshape(5, -1).sum(1).tolist() == [H * W] * 5
        pa |= {(3 * i + 1) * H * W % 4 for i in range(5)}            # image i of channel 1 of [5, 3, H, W], in floats past a 16-byte boundary
        ga |= {i * H * W % 16 for i in range(5)}
        got = cod_measures(hist.tolist(), split.tolist(), H, W)      # the host ratios of these tables: the device test adds only hist == table
        for i in range(5):
            ref = R.measures(pred[i], gt[i])
            for k in T.KEYS:
                worst = max(worst, abs(got[i][k] - ref[k]))
                assert abs(got[i][k] - ref[k]) <= 1e-12, ((H, W), i, k, got[i][k], ref[k])
    print(f"largest |table ratios - pixel ratios| on the thin batches = {worst:.3e} (bound 1e-12)")
    assert pa == {0, 1, 2, 3} and len(ga) >= 8
    below = [s for s in THIN_SHAPES if s[0] * s[1] < SPAN]
    assert len(below) >= 4 and any(h * w == SPAN for h, w in THIN_SHAPES)      # no aligned 16-byte chunk at all; exactly one
    assert {W for _, W in THIN_SHAPES} >= {1, 2, 3} and {H for H, _ in THIN_SHAPES} >= {1}      # several row wraps in a float4; one row
    big = _thin_batch((3, 341))[0]
    assert big.min() < 0 and big.max() > 1 and 3 * 341 > 3 * NT      # (more than one wave of spans, ragged: 1023 pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", THIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_histograms_and_measures_of_tiny_and_thin_images(shape):
    from camouflage_multimodal_amd import cod_measures
    pred, gt, hist, split = _thin_batch(shape)
    H, W = shape
    hn, sn = T._check_tables(pred, gt, hist, split)
    got = cod_measures(torch.from_numpy(hn), torch.from_numpy(sn), H, W)
    for i, m in enumerate(got):
        ref = R.measures(pred[i], gt[i])
        for k in T.KEYS:
            assert abs(m[k] - ref[k]) <= 1e-12, (i, k, m[k], ref[k])


# ---- 4. the weighted F-measure past one block and at the longest side ---------------------------------------------------------------

WF_KINDS = ("wide", "tall", "row", "column", "frame")


def _scatter(H, W, seed, forced=()):
    rs = np.random.RandomState(seed)
    gt = np.zeros((H, W), np.uint8)
    gt.ravel()[rs.choice(H * W, 40, replace=False)] = rs.choice([128, 200, 255], 40)
    for y, x in forced:
        gt[y, x] = 255
    return gt


@functools.lru_cache(maxsize=None)
def _wf_case(kind):
    """(pred [N, H, W], gt [N, H, W]).  wide: 9 x (SEGM_NT + 44), tall: (SEGM_NT + 44) x 3, two images each; row, column: one side of
    SEG_WF_MAX_SIDE with the one positive pixel at its end; frame: 40 x (SEGM_NT + 1), positives on all four borders."""
    side = _max_side()
    if kind == "wide":
        H, W = 9, NT + 44
        gt = np.stack([_scatter(H, W, 61, ((4, 0), (2, NT - 1), (6, NT), (4, W - 1))), _scatter(H, W, 62, ((8, NT), (0, W - 1)))])
    elif kind == "tall":
        H, W = NT + 44, 3
        gt = np.stack([_scatter(H, W, 63, ((0, 1), (H - 1, 2))), _scatter(H, W, 64)])
    elif kind == "row":
        H, W = 1, side
        gt = np.zeros((1, H, W), np.uint8)
        gt[0, 0, 0] = 255
    elif kind == "column":
        H, W = side, 1
        gt = np.zeros((1, H, W), np.uint8)
        gt[0, H - 1, 0] = 255
    else:
        H, W = 40, NT + 1
        frame = np.zeros((H, W), np.uint8)
        frame[0, 3:20] = frame[H - 1, NT - 30:] = frame[5:12, 0] = frame[20:, W - 1] = 255
        frame[16, NT // 2] = 200
        one = np.zeros((H, W), np.uint8)
        one[H - 1, W - 1] = 255
        gt = np.stack([frame, one])
    pred = np.stack([T._uniform(H, W, 70 + 10 * WF_KINDS.index(kind) + i) for i in range(len(gt))])
    return _freeze(pred, gt)


def test_the_weighted_f_cases_hold_what_their_names_say():
    side = _max_side()
    assert side % NT == 0 and TILE_X * TILE_Y == NT
    pred, gt = _wf_case("wide")
    H, W = gt.shape[1:]
    assert NT < W < 2 * NT and (gt[0] > 127).sum() in range(40, 45)
    assert all((gt[0, :, x] > 127).any() for x in (0, NT - 1, NT, W - 1)) and W % TILE_X != 0 and H % TILE_Y != 0
    assert not ((gt[0] > 127).any(0)).all()                          # columns without a positive pixel: the column pass leaves -1
    d2, idx = R.distance_transform(gt[0] > 127)
    near = idx % W                                                   # nearest pixels on both sides of the block seam, from both sides
    assert ((near[:, :NT] >= NT).any() and (near[:, NT:] < NT).any())
    pred, gt = _wf_case("tall")
    assert gt.shape[1] > NT and gt.shape[2] == 3 and (gt[1] > 127).sum() == 40
    pred, gt = _wf_case("frame")
    H, W = gt.shape[1:]
    g = gt[0] > 127
    assert W == NT + 1 and g[0].any() and g[H - 1].any() and g[:, 0].any() and g[:, W - 1].any() and g[H - 1, NT - 1] and g[H - 1, NT]
    assert (gt[1] > 127).sum() == 1 and gt[1, H - 1, W - 1] == 255
    for kind in ("row", "column"):
        pred, gt = _wf_case(kind)
        assert max(gt.shape[1:]) == side and min(gt.shape[1:]) == 1 and (gt > 127).sum() == 1
        t0 = time.perf_counter()
        sums = R.weighted_f_sums(pred[0], gt[0])
        took = time.perf_counter() - t0
        d2, idx = R.distance_transform(gt[0] > 127)
        assert d2.max() == (side - 1) ** 2 and d2.ravel()[0 if kind == "column" else -1] == d2.max() and sums[0] == 1
        assert 2.0 - math.exp(math.log(0.5) / 5.0 * (side - 1)) == 2.0       # the far end's weight has reached its limit
        assert took < 1.0, (kind, took)                              # (0.02 s where this was written: the reference stays cheap)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", WF_KINDS)
def test_weighted_f_past_one_block_and_at_the_longest_side(kind):
    pred, gt = _wf_case(kind)
    rows = WF._check(pred, gt)
    assert [r[0] for r in rows] == [int((g > 127).sum()) for g in gt]


# ---- 5. the tie rule, both halves -------------------------------------------------------------------------------------------------

TIE_KINDS = ("diagonal", "column")
TIE_SUMS = {"diagonal": ((2, 1175909819, 0), (2, 925813002, 0)), "column": ((2, 1341428705, 0), (2, 1022569326, 0))}


def _tie_case(kind):
    """(pred, gt, winner, loser): two positive pixels, the prediction 0.3 on the one the rule prefers and 1.0 on the other, 0 elsewhere.
    diagonal: 6 x 6, (0, 3) against (3, 0): the main diagonal is equidistant; the rule's (0, 3) has the smaller y' but the larger x', and
    the row pass meets (3, 0) first.  column: 7 x 5, (1, 2) against (5, 2): row 3 is equidistant, and pixel (3, 2) is decided inside its
    column."""
    (H, W), win, lose = {"diagonal": ((6, 6), (0, 3), (3, 0)), "column": ((7, 5), (1, 2), (5, 2))}[kind]
    gt, pred = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32)
    gt[win] = gt[lose] = 255
    pred[win], pred[lose] = 0.3, 1.0
    return pred, gt, win, lose


@pytest.mark.parametrize("kind", TIE_KINDS)
def test_the_tie_cases_are_tied_where_they_say(kind):
    pred, gt, win, lose = _tie_case(kind)
    H, W = gt.shape
    d2, idx = R.distance_transform(gt > 127)
    d2r, idxr = R.distance_transform(gt > 127, reverse_ties=True)
    yy, xx = np.mgrid[:H, :W]
    tied = (yy - win[0]) ** 2 + (xx - win[1]) ** 2 == (yy - lose[0]) ** 2 + (xx - lose[1]) ** 2
    assert np.array_equal(d2, d2r) and np.array_equal(idx != idxr, tied)
    assert (idx[tied] == win[0] * W + win[1]).all() and (idxr[tied] == lose[0] * W + lose[1]).all()
    if kind == "diagonal":
        assert np.array_equal(tied, np.eye(6, dtype=bool)) and win[0] < lose[0] and win[1] > lose[1]      # smaller y', LARGER x'
    else:
        assert np.array_equal(tied, yy == 3) and tied[3, 2] and win[1] == lose[1] == 2 and 3 - win[0] == lose[0] - 3
    fwd, rev = R.weighted_f_sums(pred, gt), R.weighted_f_sums(pred, gt, reverse_ties=True)
    assert (fwd, rev) == TIE_SUMS[kind]
    assert fwd[1] - rev[1] > 1000 * H * W                            # far above the bound of H * W units


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TIE_KINDS)
def test_weighted_f_tie_rule_on_the_device(kind):
    pred, gt, _, _ = _tie_case(kind)
    rows = WF._check(pred[None], gt[None])
    rev = R.weighted_f_sums(pred, gt, reverse_ties=True)
    assert abs(rows[0][1] - rev[1]) > 1000 * gt.size                 # the reversed rule is far outside the bound
