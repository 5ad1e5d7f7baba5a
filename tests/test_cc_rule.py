"""The labelling rules of csrc/cc_inl.h -- run parents, the tile unions and the border unions with what they leave out -- restated
in tests/cc_rule_ref.py and held to scipy.ndimage.label on every small input, before anything runs on a device.  CPU only."""
import numpy as np
import pytest

import cc_rule_ref as R


def all_masks(H, W):
    bits = np.arange(1 << (H * W), dtype=np.int64)[:, None] >> np.arange(H * W)[None, :]
    return (bits & 1).astype(bool).reshape(-1, H, W)


@pytest.mark.parametrize("conn", [4, 8])
def test_every_mask_of_one_tile(conn):
    """3 x 4 pixels inside one tile of side 4: the run parents and the tile rule alone."""
    m = all_masks(3, 4)
    assert len(m) == 4096
    assert np.array_equal(R.label(m, None, conn, 4), R.flood(m, None, conn))


@pytest.mark.parametrize("conn", [4, 8])
def test_every_mask_of_four_tiles(conn):
    """4 x 4 pixels in four tiles of side 2: every border, and the corner pixel that leaves out nothing."""
    m = all_masks(4, 4)
    assert len(m) == 65536
    assert np.array_equal(R.label(m, None, conn, 2), R.flood(m, None, conn))


@pytest.mark.parametrize("conn", [4, 8])
def test_label_maps_linked_on_equal_values(conn):
    """2000 random 3-value maps of 6 x 6 pixels in four tiles of side 3, every pixel a member: the equality predicate."""
    val = np.random.default_rng(20261020).integers(0, 3, size=(2000, 6, 6))
    m = np.ones(val.shape, bool)
    assert np.array_equal(R.label(m, val, conn, 3), R.flood(m, val, conn))


def test_the_three_links_are_checked_not_assumed():
    """Values 0..2 linked when they differ by at most one, 4-connectivity: three links of a square say nothing about the fourth, so
    a rule for the union above or to the left that assumed one of its three links instead of checking it fails here -- and only
    here: with an equivalence (masks, equal values) the union above and two of the links imply the third.  The diagonal rule does
    rely on an equivalence, which is why this is not run at 8."""
    near = lambda a, b: np.abs(a - b) <= 1
    val = np.random.default_rng(3).integers(0, 3, size=(2000, 6, 6))
    m = np.random.default_rng(4).random(val.shape) < 0.9
    assert np.array_equal(R.label(m, val, 4, 3, near), R.all_links(m, val, 4, near))
    assert not np.array_equal(R.all_links(m, val, 4, near), R.flood(m, val, 4))


def test_tile_side_changes_the_unions_not_the_partition():
    m = np.random.default_rng(7).random((500, 7, 9)) < 0.6
    val = np.random.default_rng(8).integers(0, 2, size=m.shape)
    want = R.flood(m, val, 8)
    kept = set()
    for T in (2, 3, 4, 16):
        assert np.array_equal(R.label(m, val, 8, T), want)
        kept.add(sum(int(c.sum()) for c in R.kept_unions(m, val, 8, T)[1].values()))
    assert len(kept) > 1
