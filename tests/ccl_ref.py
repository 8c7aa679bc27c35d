"""Fast reference for the CRAFT post-processing's labelling stage (test infrastructure), and the seeded masks and
score maps the CCL tests run on.

``label_stats`` is threshold + 4-connected labelling + per-component statistics, built on ``scipy.ndimage.label``
(default structure: 4-connected, labels in raster order of each component's first pixel) and vectorised statistics.
``tests/test_ccl_cpu.py`` pins it to ``oracle.craft_ref.connected_components`` on every topology below.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
from scipy import ndimage

F32 = np.float32

# stats: (n, 5) int32 = left, top, right, bottom, area (inclusive right/bottom); max_text: (n,) float32; row 0 = background
LabelStats = namedtuple("LabelStats", "mask flags n labels stats max_text")


def label_stats(text: np.ndarray, link: np.ndarray, low_text: float, link_thr: float) -> LabelStats:
    """cv2.threshold (strictly greater, in float32) of both maps, their union, 4-connected components numbered in
    raster order, and per component the bounding box, area and maximum text score."""
    text = np.asarray(text, F32)
    link = np.asarray(link, F32)
    t = text > F32(low_text)
    l = link > F32(link_thr)
    mask = (t | l).astype(np.uint8)
    flags = (t.astype(np.uint8) | (l.astype(np.uint8) << 1)).astype(np.uint8)
    labels, k = ndimage.label(mask)
    labels = labels.astype(np.int32)
    n = int(k) + 1
    stats = np.zeros((n, 5), np.int32)
    max_text = np.zeros((n,), F32)
    if k:
        stats[:, 4] = np.bincount(labels.ravel(), minlength=n)
        stats[0, 4] = 0
        for i, sl in enumerate(ndimage.find_objects(labels, max_label=k), start=1):
            stats[i, :4] = (sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1)
        max_text[1:] = ndimage.maximum(text, labels, index=np.arange(1, n)).astype(F32)
    return LabelStats(mask, flags, n, labels, stats, max_text)


def cv_components(ls: LabelStats):
    """(n, labels, stats[n,5] = left, top, width, height, area): what ``craft_ref.connected_components`` returns."""
    s = ls.stats.astype(np.int64)
    cv = np.stack([s[:, 0], s[:, 1], s[:, 2] - s[:, 0] + 1, s[:, 3] - s[:, 1] + 1, s[:, 4]], axis=1)
    cv[0] = 0
    return ls.n, ls.labels, cv


# ----------------------------------------------------------------------------------------------------------- masks
def _spiral(H, W):
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and not m[yy, xx]

    def can(dy, dx):   # the next cell is free, and the one after it is not part of an earlier lap
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        return free(y1, x1) and (not (0 <= y2 < H and 0 <= x2 < W) or not m[y2, x2])

    while True:
        if not can(dy, dx):
            dy, dx = dx, -dy       # turn right (y down)
            if not can(dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = True
    return m


def _w_shape(H, W):
    """Four 4-connected slanted strokes \\/\\/ : the first raster pixel is the top of the left arm, the arms join only
    through the short runs at the bottom vertices."""
    m = np.zeros((H, W), bool)
    L = H - 2
    k = max(1, math.ceil(4 * L / max(W - 4, 1)))   # rows per column step
    x0 = 1
    for stroke in range(4):
        for t in range(L):
            y = 1 + t if stroke % 2 == 0 else L - t
            xa, xb = x0 + t // k, x0 + (t + 1) // k
            m[y, min(xa, W - 1)] = True
            m[y, min(xb, W - 1)] = True
        x0 += L // k
    return m


def _rings(H, W, count=4, step=3):
    m = np.zeros((H, W), bool)
    for r in range(count):
        a = r * step
        if H - 1 - a <= a or W - 1 - a <= a:
            break
        m[a, a:W - a] = True
        m[H - 1 - a, a:W - a] = True
        m[a:H - a, a] = True
        m[a:H - a, W - 1 - a] = True
    return m


TOPOLOGIES = ("empty", "full", "corners", "checkerboard", "hstripes", "vstripes", "comb", "inverted_comb", "serpentine",
              "spiral", "staircase", "w", "rings", "random_0.3", "random_0.5", "random_0.593", "random_0.8")


def topology(name: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """Boolean (H, W) mask of the named topology."""
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "empty":
        return np.zeros((H, W), bool)
    if name == "full":
        return np.ones((H, W), bool)
    if name == "corners":
        m = np.zeros((H, W), bool)
        m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
        return m
    if name == "checkerboard":
        return (yy + xx) % 2 == 0
    if name == "hstripes":
        return yy % 2 == 0
    if name == "vstripes":
        return xx % 2 == 0
    if name == "comb":            # teeth joined only along the last row
        return (xx % 2 == 0) | (yy == H - 1)
    if name == "inverted_comb":   # teeth hanging from the first row
        return (xx % 2 == 0) | (yy == 0)
    if name == "serpentine":      # full even rows, joined alternately at the right and the left end: one path of ~n/2
        turn = np.where((yy // 2) % 2 == 0, W - 1, 0)
        return (yy % 2 == 0) | (xx == turn)
    if name == "spiral":
        return _spiral(H, W)
    if name == "staircase":       # 3x3 blocks that touch only at their corners
        m = np.zeros((H, W), bool)
        for x0 in range(0, W, 9):
            for i in range(H // 3 + 1):
                m[3 * i:3 * i + 3, x0 + 3 * i:x0 + 3 * i + 3] = True
        return m
    if name == "w":
        return _w_shape(H, W)
    if name == "rings":
        return _rings(H, W)
    if name.startswith("random_"):
        return np.random.default_rng(seed + 1000).random((H, W)) < float(name.split("_")[1])
    raise KeyError(name)


def width_mask(W: int, variant: str = "random", H: int = 5, seed: int = 0) -> np.ndarray:
    """Seeded random 0.6 with forced runs over columns 250-262 and 505-520 (where they fit); the variants force the
    256-column chunk boundary: "bg255" = column 255 background, 256 foreground; "fg255" = the reverse."""
    m = np.random.default_rng(seed + 7 * W).random((H, W)) < 0.6
    m[2, 250:263] = True
    m[3, 505:521] = True
    if variant == "bg255":
        m[:, 255:256] = False
        m[:, 256:257] = True
    elif variant == "fg255":
        m[:, 255:256] = True
        m[:, 256:257] = False
    elif variant != "random":
        raise KeyError(variant)
    return m


def scan_mask(H: int, W: int, force=(2047, 2048), seed: int = 0) -> np.ndarray:
    """Seeded random 0.5 around the seam of the first two 2048-pixel scan blocks.  The pixels at the flat indices in
    ``force`` are set and the left and upper neighbours of the first of them cleared, so that pixel is the first of its
    component: a root right at the seam (2047, 2048) or in the last, partly filled block (2046 of n = 2047)."""
    n = H * W
    assert all(0 <= i < n for i in force)
    m = np.random.default_rng(seed + n).random(n) < 0.5
    for i in range(min(force) - 1, max(force) + 2):
        for j in (i, i - W):
            if 0 <= j < n:
                m[j] = False
    m[list(force)] = True
    return m.reshape(H, W)


# (shape, forced flat indices): n = 2047, 2048 and 2049 pixels in two shapes each, every distinct placement of a root
SCAN_CASES = [((1, 2047), (2046,)), ((23, 89), (2046,)), ((1, 2048), (2047,)), ((32, 64), (2047,)),
              ((1, 2049), (2047,)), ((1, 2049), (2048,)), ((1, 2049), (2047, 2048)),
              ((3, 683), (2047,)), ((3, 683), (2048,)), ((3, 683), (2047, 2048))]


def large_mask(H: int = 1025, W: int = 2049, seed: int = 0, band_rows: int = 40, band_density: float = 0.3):
    """A serpentine over the left half, 200 seeded rectangles over the right half, a random band in the last rows."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), bool)
    top = H - band_rows - 1
    half = W // 2
    m[:top, :half] = topology("serpentine", top, half)
    for _ in range(200):
        h, w = int(rng.integers(2, 60)), int(rng.integers(2, 120))
        y, x = int(rng.integers(0, top - h)), int(rng.integers(half + 2, W - w + 1))
        m[y:y + h, x:x + w] = True
    m[H - band_rows:, :] = rng.random((band_rows, W)) < band_density
    return m


def tall_mask(H: int = 1_050_001, W: int = 3, seed: int = 0) -> np.ndarray:
    """A tall narrow map: seeded vertical runs (1-200 rows, one of 3000) in the outer columns, sparse bridges between
    them in the middle one.  One-pixel runs per row, tall parent chains, components in the tens of thousands."""
    rng = np.random.default_rng(seed + 5)
    m = np.zeros((H, W), bool)
    for c in (0, W - 1):
        lens = rng.integers(1, 201, size=2 * H // 100 + 16)
        if c == 0:
            lens[10] = 3000
        edges = np.cumsum(lens)
        on = (np.searchsorted(edges, np.arange(H), side="right") % 2) == 0
        m[:, c] = on
    if W > 2:
        m[:, 1:W - 1] = rng.random((H, W - 2)) < 0.02
    return m


# ------------------------------------------------------------------------------------------------------ score maps
def scores_from_masks(mask_t: np.ndarray, mask_l: np.ndarray, low_text: float, link_thr: float, seed: int = 0,
                      margin: float = 0.05) -> np.ndarray:
    """(H, W, 2) fp32: text = mask_t ? hi : lo with hi / lo at least ``margin`` from low_text, and likewise link.  Every
    pixel's text score is a distinct value (a seeded permutation of an arithmetic grid)."""
    H, W = mask_t.shape
    n = H * W
    r = (np.random.default_rng(seed + 17).permutation(n).astype(np.float64) / n).reshape(H, W)
    text = np.where(mask_t, low_text + margin + 0.4 * r, low_text - margin - 0.2 * r).astype(F32)
    link = np.where(mask_l, link_thr + margin + 0.3 * r, link_thr - margin - 0.3 * r).astype(F32)
    return np.ascontiguousarray(np.stack([text, link], axis=2))


def rotated_rect_mask(H: int, W: int, cx: float, cy: float, length: float, thick: float, deg: float) -> np.ndarray:
    """Pixels whose centre lies inside the rectangle of the given centre, side lengths and rotation."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    u = (xx - cx) * c + (yy - cy) * s
    v = -(xx - cx) * s + (yy - cy) * c
    return (np.abs(u) <= length / 2) & (np.abs(v) <= thick / 2)


# ------------------------------------------------------------------------------------------- designed box-stage maps
SPARSE = (0.7, 0.45, 0.3)      # text_threshold, link_threshold, low_text of BoxProcessorCraft's "sparse" mode
RAW_LINE = (0.4, 0.2, 0.5)     # "raw_line": text_threshold below low_text


def expected_niter(size: int, w: int, h: int) -> int:
    """craft_utils.py:62: int(math.sqrt(size * min(w, h) / (w * h)) * 2)"""
    return int(math.sqrt(size * min(w, h) / (w * h)) * 2)


class _Canvas:
    """Score maps under construction: background everywhere, blobs painted with seeded distinct text scores."""

    def __init__(self, H, W, thresholds, seed):
        self.tt, self.lt, self.low = thresholds
        self.rng = np.random.default_rng(seed)
        n = H * W
        r = (self.rng.permutation(n).astype(np.float64) / n).reshape(H, W)
        self.r = r
        self.text = (min(self.low, self.tt) - 0.1 - 0.1 * r).astype(F32)    # below both text thresholds
        self.link = np.full((H, W), self.lt - 0.1, F32)

    def text_blob(self, mask, lo=None, hi=None):
        """text scores in [lo, hi]: by default above text_threshold by 0.05 or more"""
        lo = max(self.tt, self.low) + 0.05 if lo is None else lo
        hi = lo + 0.2 if hi is None else hi
        self.text[mask] = (lo + (hi - lo) * self.r[mask]).astype(F32)

    def link_blob(self, mask):
        self.link[mask] = F32(self.lt + 0.1)

    def scores(self):
        return np.ascontiguousarray(np.stack([self.text, self.link], axis=2))


def _rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


BOX_CASES = ("axis_bars", "rotated_bars", "align", "area_9_10", "low_text_max", "link_only", "bridge", "thin_l", "grid_5x5")


def box_case(name: str):
    """-> (scores (H, W, 2) fp32, (text_threshold, link_threshold, low_text), designed number of boxes)"""
    if name == "axis_bars":      # one bar on each border, one in two corners, one inside: sx, sy, ex, ey all clipped
        H, W = 96, 160
        c = _Canvas(H, W, SPARSE, 1)
        for y0, y1, x0, x1 in ((0, 4, 40, 81), (92, 96, 30, 71), (30, 61, 0, 4), (30, 61, 156, 160), (0, 5, 0, 21),
                               (88, 96, 140, 160), (45, 51, 60, 111)):
            c.text_blob(_rect(H, W, y0, y1, x0, x1))
        return c.scores(), SPARSE, 7
    if name == "rotated_bars":   # 40 x 8 at five angles, centres jittered off the pixel grid
        H, W = 128, 192
        c = _Canvas(H, W, SPARSE, 2)
        for (cy, cx), deg in zip(((32, 32), (32, 96), (32, 160), (96, 48), (96, 144)), (15, 30, 45, 60, 80)):
            jy, jx = c.rng.random(2) - 0.5
            c.text_blob(rotated_rect_mask(H, W, cx + jx, cy + jy, 40.0, 8.0, deg))
        return c.scores(), SPARSE, 5
    if name == "align":          # a near-square blob turned by 10 degrees, a diamond (both within 0.1 of square) and a 30-degree bar of ratio 1.14
        H, W = 96, 176
        c = _Canvas(H, W, SPARSE, 3)
        c.text_blob(rotated_rect_mask(H, W, 22.3, 40.2, 22.0, 21.0, 10.0))
        c.text_blob(rotated_rect_mask(H, W, 88.3, 48.2, 24.0, 24.0, 45.0))
        c.text_blob(rotated_rect_mask(H, W, 145.4, 47.7, 29.0, 24.0, 30.0))
        return c.scores(), SPARSE, 3
    if name == "area_9_10":      # 3 x 3 is dropped (size < 10), 2 x 5 is kept
        H, W = 48, 64
        c = _Canvas(H, W, SPARSE, 4)
        c.text_blob(_rect(H, W, 10, 13, 10, 13))
        c.text_blob(_rect(H, W, 30, 32, 40, 45))
        return c.scores(), SPARSE, 1
    if name == "low_text_max":   # big enough, but its best text score stays 0.01 under text_threshold
        H, W = 64, 96
        c = _Canvas(H, W, SPARSE, 5)
        c.text_blob(_rect(H, W, 10, 18, 10, 40), lo=SPARSE[2] + 0.05, hi=SPARSE[0] - 0.01)
        c.text_blob(_rect(H, W, 40, 48, 50, 80))
        return c.scores(), SPARSE, 1
    if name == "link_only":      # text in (text_threshold, low_text): labelled through the link map only, passes the text
        H, W = 64, 96           # test, and its whole segmap is removed -> the zero box.  Plus one ordinary blob.
        c = _Canvas(H, W, RAW_LINE, 6)
        m = _rect(H, W, 10, 16, 10, 40)
        c.link_blob(m)
        c.text_blob(m, lo=RAW_LINE[0] + 0.02, hi=RAW_LINE[2] - 0.05)
        c.text_blob(_rect(H, W, 40, 48, 50, 80))
        return c.scores(), RAW_LINE, 2
    if name == "bridge":         # two text blobs joined by a link-only bridge: one label, the bridge leaves the segmap
        H, W = 64, 128
        c = _Canvas(H, W, SPARSE, 7)
        c.text_blob(_rect(H, W, 20, 32, 10, 40))
        c.text_blob(_rect(H, W, 24, 40, 80, 110))
        c.link_blob(_rect(H, W, 27, 30, 40, 80))
        return c.scores(), SPARSE, 1
    if name == "thin_l":         # 30 x 1 plus 1 x 30
        H, W = 64, 64
        c = _Canvas(H, W, SPARSE, 8)
        c.text_blob(_rect(H, W, 15, 45, 20, 21) | _rect(H, W, 44, 45, 20, 50))
        return c.scores(), SPARSE, 1
    if name == "grid_5x5":       # 25 bars over two 256-column chunks: label order
        H, W = 64, 300
        c = _Canvas(H, W, SPARSE, 9)
        for i in range(5):
            for j in range(5):
                c.text_blob(_rect(H, W, 4 + 12 * i, 6 + 12 * i, 10 + 58 * j, 40 + 58 * j))
        return c.scores(), SPARSE, 25
    raise KeyError(name)
