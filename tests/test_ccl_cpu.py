"""The fast labelling reference of the CCL tests (tests/ccl_ref.py, scipy.ndimage) pinned to the oracle's restatement of
cv2.connectedComponentsWithStats (oracle/craft_ref.py, cross-checked in tests/test_oracle_craft.py): same count, same
raster-order numbering, same statistics, on every topology the GPU tests use, at its small size.  Also checks on the CPU
that every designed box-stage map yields the designed number of boxes.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccl_ref as R  # noqa: E402
from oracle import craft_ref  # noqa: E402

LOW, LINK = 0.3, 0.45


def _check_against_oracle(mask_t, mask_l):
    sc = R.scores_from_masks(mask_t, mask_l, LOW, LINK, seed=3)
    text, link = sc[:, :, 0], sc[:, :, 1]
    assert (np.abs(text - np.float32(LOW)) >= 0.05 - 1e-6).all() and (np.abs(link - np.float32(LINK)) >= 0.05 - 1e-6).all()
    assert len(np.unique(text)) == text.size, "text scores are not distinct"
    ls = R.label_stats(text, link, LOW, LINK)
    np.testing.assert_array_equal(ls.mask.astype(bool), mask_t | mask_l)
    np.testing.assert_array_equal(ls.flags, mask_t.astype(np.uint8) + 2 * mask_l.astype(np.uint8))
    n, labels, stats = craft_ref.connected_components(ls.mask)
    assert ls.n == n
    np.testing.assert_array_equal(ls.labels, labels)
    got_n, got_labels, got_stats = R.cv_components(ls)
    assert got_n == n and got_labels is ls.labels
    np.testing.assert_array_equal(got_stats[1:], stats[1:])
    for k in range(1, n):   # the maximum, by the definition
        assert ls.max_text[k] == text[labels == k].max()
    return ls


@pytest.mark.parametrize("name", R.TOPOLOGIES)
def test_fast_reference_equals_oracle_on_topology(name):
    m = R.topology(name, 33, 65)
    ls = _check_against_oracle(m, np.zeros_like(m))
    if name == "empty":
        assert ls.n == 1
    else:
        assert ls.n > 1
    if name == "checkerboard":
        assert ls.n - 1 == (33 * 65) // 2 + 1
    if name in ("full", "comb", "inverted_comb", "serpentine", "spiral", "w"):
        assert ls.n == 2
    if name == "rings":
        assert ls.n == 5
    if name == "serpentine":
        assert m.sum() >= 33 * 65 // 2


@pytest.mark.parametrize("W,variant", [(9, "random"), (257, "random"), (257, "bg255"), (257, "fg255"), (513, "random")])
def test_fast_reference_equals_oracle_on_width_masks(W, variant):
    m = R.width_mask(W, variant)
    _check_against_oracle(m, np.zeros_like(m))


@pytest.mark.parametrize("hw,force", R.SCAN_CASES)
def test_scan_masks_have_a_root_at_the_seam(hw, force):
    m = R.scan_mask(*hw, force=force)
    assert m.ravel()[list(force)].all()
    ls = _check_against_oracle(m, np.zeros_like(m))
    k = ls.labels.ravel()[force[0]]
    assert k > 0 and np.flatnonzero(ls.labels.ravel() == k)[0] == force[0]


def test_scan_cases_are_distinct_masks():
    masks = {(hw, R.scan_mask(*hw, force=force).tobytes()) for hw, force in R.SCAN_CASES}
    assert len(masks) == len(R.SCAN_CASES) == 10


def test_fast_reference_equals_oracle_with_independent_link_mask():
    rng = np.random.default_rng(11)
    mt, ml = rng.random((33, 65)) < 0.35, rng.random((33, 65)) < 0.35
    ls = _check_against_oracle(mt, ml)
    assert set(np.unique(ls.flags)) == {0, 1, 2, 3}


@pytest.mark.parametrize("name", R.BOX_CASES)
def test_designed_box_maps_yield_the_designed_boxes(name):
    """get_det_boxes with the fast labeller's components equals get_det_boxes with its own, and gives the designed count."""
    sc, (tt, lt, low), designed = R.box_case(name)
    text, link = sc[:, :, 0], sc[:, :, 1]
    ls = R.label_stats(text, link, low, lt)
    fast, _, fast_map = craft_ref.get_det_boxes(text, link, tt, lt, low, components=R.cv_components(ls))
    slow, _, slow_map = craft_ref.get_det_boxes(text, link, tt, lt, low)
    assert len(fast) == len(slow) == designed >= 1
    assert fast_map == slow_map
    np.testing.assert_array_equal(np.stack(fast), np.stack(slow))
    # every surviving maximum is clear of text_threshold, every dropped one too
    assert (np.abs(ls.max_text[1:].astype(np.float64) - tt) >= 1e-3).all()
