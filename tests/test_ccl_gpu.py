"""Kernel-level tests of the CRAFT post-processing (csrc/ccl.hip and the box stage of csrc/craft_api.hip) through
``mhip_craft_boxes_host``: the shipped post-processing on a designed score map, no network, no weights.

Labelling and statistics are integer work: labels, flags and all six statistics are compared with ``assert_array_equal``
against tests/ccl_ref.py (scipy.ndimage, pinned to the oracle in tests/test_ccl_cpu.py), the maximum text score bit for
bit.  Boxes are compared with ``assert_array_equal`` against ``oracle.craft_ref.get_det_boxes`` on the same map, order
included.  The labelling cases pass a text threshold no score reaches, so they spend no time in the box loop.

What each case is there for (lines of csrc/ccl.hip):

| case | kernel | lines |
|---|---|---|
| widths 1, 7, 8, 9 | ``ccl_stats_kernel``: 8-pixel segments, flush at the segment's end | 197-231 |
| widths 63, 64, 65 | ``ccl_rows_kernel``: 64-lane max-scan and the ``wmax`` hand-over between waves | 44-52 |
| widths 255, 256, 257, 513, bg255 / fg255 | ``ccl_rows_kernel``: ``carry_s`` over one and two 256-column chunks, run head on either side | 34, 50-56 |
| scan n = 2047, 2048, 2049 | ``ccl_count_roots_kernel`` / ``ccl_rank_roots_kernel``: the ``i < n`` edge and the block offset of a root at a block seam | 129-130, 171-183 |
| empty, full, corners | ``ccl_scan_blocks_kernel`` total, ``ccl_init_stats_kernel`` | 161, 237 |
| checkerboard (odd n) | statistics capacity ``n/2 + 2`` rows | 266, 288 |
| stripes, comb, inverted comb | ``ccl_merge_kernel``: one union per contact segment; ``unite`` under contention on one root | 69-94 |
| vertical stripes, serpentine, spiral | ``find_root`` on long parent chains, ``ccl_compress_heads_kernel`` | 60-66, 101-107 |
| staircase | diagonal contact is no contact | 90-92 |
| W, rings | a root that is not on the joining run; ``ccl_flatten_kernel`` | 79-81, 117 |
| random 0.3 - 0.8 | all of the above at once; 0.593 is the site-percolation threshold | |
| flags | ``ccl_rows_kernel`` binarise | 39 |
| negative text | ``float_to_ordered`` negative branch, ``mhip_ordered_bits_to_float`` | 19, 252 |
| threshold edge | strict ``>`` in float32 | 39 |
| large 1025 x 2049 | grid-stride loops of merge / compress / flatten (n > 1 048 576 threads); ``per == 2`` in ``ccl_scan_blocks_kernel`` (1026 blocks) | 89, 101, 114, 143-160 |
| tall 1 050 001 x 3 | grid-stride loop of ``ccl_stats_kernel``, which strides over H * ceil(W / 8) segments, not pixels (1 050 001 > 1 048 576); the other strides and ``per == 2`` again; a 3000-row parent chain | 195-196, 62-65 |
| run-to-run | the racing ``atomicMin`` unions and statistics atomics give one result | 79, 214-219 |

Box stage (csrc/craft_api.hip, ``craft_boxes``): border clipping of the dilation window, rotated minimum-area rectangles,
the diamond-align branch and its edge, the ``size < 10`` and text-threshold filters, the all-link-only zero box, segmap
removal of link-only pixels, the smallest ``niter``, and label order across chunks.

``niter == 0`` (``ks == 1``, no dilation) cannot be reached: a 4-connected component of bounding box w x h has at least
w + h - 1 pixels, so size * min(w, h) / (w * h) >= (w + h - 1) / max(w, h) >= 1 and ``niter`` >= 2.  The thin "L" is the
component closest to that bound; its test asserts ``niter == 2``.

The zero box needs a component whose text passes ``text_threshold`` nowhere above ``low_text``, so it needs
``text_threshold <= low_text``: of ``BoxProcessorCraft._THRESHOLDS`` only "raw_line" (0.4, 0.2, 0.5) reaches it, and the
case uses that triple.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccl_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
LOW, LINK = 0.3, 0.45
NO_BOXES = 10.0   # a text threshold no score reaches: labelling cases skip the box loop


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _run(ctx, scores, tt=NO_BOXES, link=LINK, low=LOW, max_boxes=4096):
    from marie_icr_amd.craft import craft_boxes

    return craft_boxes(ctx, scores, tt, link, low, max_boxes=max_boxes)


def _assert_labelling(got, ref, what=""):
    """n_labels, labels, flags and the six statistics of labels 1..n-1, all exact."""
    if got["n_labels"] != ref.n or not np.array_equal(got["labels"], ref.labels):
        bad = np.argwhere(got["labels"] != ref.labels)[:20]
        print(f"{what}: n_labels {got['n_labels']} vs {ref.n}; first mismatching pixels (y, x, got, ref):")
        for y, x in bad:
            print(int(y), int(x), int(got["labels"][y, x]), int(ref.labels[y, x]))
    assert got["n_labels"] == ref.n, what
    np.testing.assert_array_equal(got["flags"], ref.flags, err_msg=what)
    np.testing.assert_array_equal(got["labels"], ref.labels, err_msg=what)
    np.testing.assert_array_equal(got["stats"][1:], ref.stats[1:], err_msg=what)
    np.testing.assert_array_equal(got["max_text"][1:].view(np.int32), ref.max_text[1:].view(np.int32), err_msg=what)


def _check_mask(ctx, mask, what, seed=0):
    sc = R.scores_from_masks(mask, np.zeros_like(mask), LOW, LINK, seed=seed)
    ref = R.label_stats(sc[:, :, 0], sc[:, :, 1], LOW, LINK)
    np.testing.assert_array_equal(ref.mask.astype(bool), mask)
    got = _run(ctx, sc)
    _assert_labelling(got, ref, what)
    assert len(got["boxes"]) == 0
    return got, ref


# ------------------------------------------------------------------------------------------- labelling and statistics
WIDTHS = [(w, "random") for w in (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513)] + \
         [(w, v) for w in (257, 513) for v in ("bg255", "fg255")]


@pytest.mark.parametrize("W,variant", WIDTHS)
def test_widths(ctx, W, variant):
    m = R.width_mask(W, variant)
    if variant == "bg255":
        assert not m[:, 255].any() and m[:, 256].all()
    if variant == "fg255":
        assert m[:, 255].all() and not m[:, 256].any()
    _, ref = _check_mask(ctx, m, f"W={W} {variant}")
    assert ref.n > 1


@pytest.mark.parametrize("hw,force", R.SCAN_CASES)
def test_scan_block_seam(ctx, hw, force):
    m = R.scan_mask(*hw, force=force)
    _, ref = _check_mask(ctx, m, f"{hw} {force}")
    k = ref.labels.ravel()[force[0]]   # the first forced pixel is a root
    assert k > 0 and np.flatnonzero(ref.labels.ravel() == k)[0] == force[0]


@pytest.mark.parametrize("hw", [(33, 65), (64, 300)])
@pytest.mark.parametrize("name", R.TOPOLOGIES)
def test_topology(ctx, name, hw):
    m = R.topology(name, *hw)
    n = hw[0] * hw[1]
    ref = R.label_stats(m.astype(np.float32), np.zeros(hw, np.float32), 0.5, 0.5)
    if name == "empty":
        assert ref.n == 1
    elif name == "checkerboard":
        assert ref.n - 1 == (n // 2 + 1 if n % 2 else n // 2)   # odd n: the capacity of the statistics buffer
    elif name in ("full", "comb", "inverted_comb", "serpentine", "spiral", "w"):
        assert ref.n == 2
    elif name == "rings":
        assert ref.n == 5
    else:
        assert ref.n > 2
    got, _ = _check_mask(ctx, m, f"{name} {hw}")
    if name == "empty":
        assert got["n_labels"] == 1 and not got["labels"].any()


def test_flags_all_four(ctx):
    rng = np.random.default_rng(21)
    mt, ml = rng.random((64, 300)) < 0.35, rng.random((64, 300)) < 0.35
    sc = R.scores_from_masks(mt, ml, LOW, LINK, seed=5)
    ref = R.label_stats(sc[:, :, 0], sc[:, :, 1], LOW, LINK)
    assert set(np.unique(ref.flags)) == {0, 1, 2, 3} and ref.n > 100
    _assert_labelling(_run(ctx, sc), ref, "flags")


def test_negative_text_scores(ctx):
    """A link-only component over negative text scores: the statistic is the most positive of the negatives, exactly.  A
    second link-only component holds both signs."""
    H, W = 24, 300
    rng = np.random.default_rng(22)
    text = (-(0.05 + rng.permutation(H * W) / (H * W))).astype(np.float32).reshape(H, W)
    link = np.full((H, W), LINK - 0.1, np.float32)
    link[3:9, 20:280] = LINK + 0.1
    link[14:20, 40:90] = LINK + 0.1
    text[14:20, 40:90:2] *= np.float32(-0.2)      # positive, still under low_text
    sc = np.ascontiguousarray(np.stack([text, link], axis=2))
    ref = R.label_stats(text, link, LOW, LINK)
    assert ref.n == 3 and set(np.unique(ref.flags)) == {0, 2}
    assert ref.max_text[1] == text[3:9, 20:280].max() < 0 < ref.max_text[2] < LOW
    _assert_labelling(_run(ctx, sc), ref, "negative text")


def test_threshold_edge(ctx):
    """cv2.threshold is strictly greater, in float32: a score equal to the threshold is background, the next float is not."""
    H, W = 8, 16
    text = np.full((H, W), LOW - 0.1, np.float32)
    link = np.full((H, W), LINK - 0.1, np.float32)
    text[2, 3] = np.float32(LOW)
    text[2, 8] = np.nextafter(np.float32(LOW), np.float32(np.inf))
    link[5, 3] = np.float32(LINK)
    link[5, 8] = np.nextafter(np.float32(LINK), np.float32(np.inf))
    sc = np.ascontiguousarray(np.stack([text, link], axis=2))
    ref = R.label_stats(text, link, LOW, LINK)
    assert ref.n == 3 and ref.flags[2, 3] == 0 and ref.flags[2, 8] == 1 and ref.flags[5, 3] == 0 and ref.flags[5, 8] == 2
    got = _run(ctx, sc)
    _assert_labelling(got, ref, "threshold edge")
    assert got["flags"][2, 3] == 0 and got["flags"][2, 8] == 1 and got["flags"][5, 3] == 0 and got["flags"][5, 8] == 2


def test_large_map(ctx):
    """1025 x 2049 = 2 100 225 pixels: more than the capped grids cover in one stride (1 048 576) and more than 1024 scan
    blocks (per == 2)."""
    m = R.large_mask()
    assert m.size > 2 * 1024 * 1024 and m.shape == (1025, 2049)
    sc = R.scores_from_masks(m, np.zeros_like(m), LOW, LINK, seed=9)
    ref = R.label_stats(sc[:, :, 0], sc[:, :, 1], LOW, LINK)
    assert 5000 < ref.n < 40000
    t0 = time.perf_counter()
    got = _run(ctx, sc)
    print(f"large map: {ref.n - 1} components, mhip_craft_boxes_host {time.perf_counter() - t0:.3f} s")
    _assert_labelling(got, ref, "large")


def test_tall_map(ctx):
    """1 050 001 x 3: one 8-pixel statistics segment per row, so ccl_stats_kernel has more segments than the capped grid
    has threads (4096 x 256) and strides; 3 150 003 pixels stride the other kernels and give per == 2."""
    m = R.tall_mask()
    H, W = m.shape
    assert H * ((W + 7) // 8) > 4096 * 256 and m.size > 2 * 1024 * 1024
    sc = R.scores_from_masks(m, np.zeros_like(m), LOW, LINK, seed=4)
    ref = R.label_stats(sc[:, :, 0], sc[:, :, 1], LOW, LINK)
    assert 5000 < ref.n < 40000 and (ref.stats[1:, 3] - ref.stats[1:, 1]).max() >= 3000
    assert ref.labels[4096 * 256:].any()   # components whose statistics come from a second stride only
    t0 = time.perf_counter()
    got = _run(ctx, sc)
    print(f"tall map: {ref.n - 1} components, mhip_craft_boxes_host {time.perf_counter() - t0:.3f} s")
    _assert_labelling(got, ref, "tall")


@pytest.mark.parametrize("name", ["random_0.593", "comb"])
def test_run_to_run_stability(ctx, name):
    m = R.topology(name, 64, 300)
    sc = R.scores_from_masks(m, np.zeros_like(m), LOW, LINK, seed=1)
    ref = R.label_stats(sc[:, :, 0], sc[:, :, 1], LOW, LINK)
    assert ref.n > 1
    for it in range(20):
        _assert_labelling(_run(ctx, sc), ref, f"{name} run {it}")


def test_small_statistics_capacity_is_an_error(ctx):
    from marie_icr_amd._lib import MarieHipError, check

    m = R.topology("corners", 9, 9)
    sc = R.scores_from_masks(m, np.zeros_like(m), LOW, LINK)
    stats = np.zeros((4, 6), np.int32)   # 5 labels with the background
    nb, nl = C.c_int(), C.c_int()
    rc = ctx.lib.mhip_craft_boxes_host(ctx.h, sc.ctypes.data_as(C.c_void_p), 9, 9, NO_BOXES, LINK, LOW, C.c_void_p(0), 0,
                                       C.byref(nb), C.c_void_p(0), C.c_void_p(0), stats.ctypes.data_as(C.c_void_p), 4,
                                       C.byref(nl))
    assert rc != 0 and nl.value == 5 and not stats.any()
    with pytest.raises(MarieHipError, match="statistics capacity"):
        check(ctx.h, rc, "mhip_craft_boxes_host")


# ---------------------------------------------------------------------------------------------------------- box stage
def _box_case(ctx, name):
    from oracle import craft_ref

    sc, (tt, lt, low), designed = R.box_case(name)
    text, link = sc[:, :, 0], sc[:, :, 1]
    ref = R.label_stats(text, link, low, lt)
    assert (np.abs(ref.max_text[1:].astype(np.float64) - tt) >= 1e-3).all()
    ref_boxes, _, mapper = craft_ref.get_det_boxes(text, link, tt, lt, low, components=R.cv_components(ref))
    assert len(ref_boxes) == designed >= 1, (name, len(ref_boxes))
    ref_boxes = np.stack(ref_boxes).astype(np.float32)
    got = _run(ctx, sc, tt, lt, low)
    _assert_labelling(got, ref, name)
    assert got["boxes"].shape == ref_boxes.shape, (name, got["boxes"].shape)
    np.testing.assert_array_equal(got["boxes"], ref_boxes, err_msg=name)
    return got, ref, ref_boxes, mapper


def _axis_aligned(box):
    return box[0, 1] == box[1, 1] and box[1, 0] == box[2, 0] and box[2, 1] == box[3, 1] and box[3, 0] == box[0, 0]


def _side_ratio(box):
    a, b = np.linalg.norm(box[0] - box[1]), np.linalg.norm(box[1] - box[2])
    return max(a, b) / min(a, b)


@pytest.mark.parametrize("name", ["axis_bars", "rotated_bars", "area_9_10", "low_text_max", "grid_5x5"])
def test_boxes(ctx, name):
    got, ref, boxes, mapper = _box_case(ctx, name)
    if name == "axis_bars":      # the dilation window was clipped on every side
        H, W = ref.labels.shape
        assert boxes[:, :, 0].min() == 0 and boxes[:, :, 1].min() == 0
        assert boxes[:, :, 0].max() == W - 1 and boxes[:, :, 1].max() == H - 1
    if name == "rotated_bars":
        assert not any(_axis_aligned(b) for b in boxes)
    if name == "area_9_10":
        assert sorted(ref.stats[1:, 4].tolist()) == [9, 10] and ref.stats[mapper[0], 4] == 10
    if name == "low_text_max":
        assert ref.n == 3 and (ref.stats[1:, 4] >= 10).all()
    if name == "grid_5x5":
        assert mapper == list(range(1, 26))


def test_boxes_align_branch(ctx):
    """The near-square blob (turned by 10 degrees) and the diamond take the align branch: the minimum-area rectangle of
    either is not axis-aligned, the box is, and it is the extremes of the dilated pixels.  The 30-degree bar of side
    ratio 1.14 does not take it."""
    from oracle import craft_ref

    _, ref, boxes, mapper = _box_case(ctx, "align")
    order = np.argsort(boxes[:, :, 0].min(axis=1))
    by_x = boxes[order]
    for j in (0, 1):
        k = mapper[order[j]]
        ys, xs = np.nonzero(ref.labels == k)
        assert not _axis_aligned(craft_ref.min_area_rect_box(np.stack([xs, ys], axis=1)))
        assert _axis_aligned(by_x[j])
        l, t, r, b, size = (int(v) for v in ref.stats[k])
        a = (1 + R.expected_niter(size, r - l + 1, b - t + 1)) // 2   # the ks x ks dilation reaches ks // 2 each way
        np.testing.assert_array_equal(by_x[j], np.array([[l - a, t - a], [r + a, t - a], [r + a, b + a], [l - a, b + a]],
                                                        np.float32))
    assert not _axis_aligned(by_x[2]) and 1.1 < _side_ratio(by_x[2]) < 1.2


def test_boxes_link_only_component_gives_the_zero_box(ctx):
    _, ref, boxes, mapper = _box_case(ctx, "link_only")
    k = mapper[0]
    assert (ref.flags[ref.labels == k] == 2).all() and ref.stats[k, 4] >= 10
    assert not boxes[0].any() and boxes[1].any()


def test_boxes_link_bridge(ctx):
    _, ref, boxes, _ = _box_case(ctx, "bridge")
    assert ref.n == 2 and set(np.unique(ref.flags[ref.labels == 1])) == {1, 2}


def test_boxes_thin_l_smallest_niter(ctx):
    _, ref, boxes, _ = _box_case(ctx, "thin_l")
    l, t, r, b, size = (int(v) for v in ref.stats[1])
    assert (r - l + 1, b - t + 1, size) == (30, 30, 59)
    assert R.expected_niter(size, 30, 30) == 2   # the smallest a connected component can have: see the module docstring
    np.testing.assert_array_equal(boxes[0], np.array([[l - 1, t - 1], [r + 1, t - 1], [r + 1, b + 1], [l - 1, b + 1]], np.float32))
