"""The VQ-NNF kernels (csrc/vqnnf.hip) and ``VQNNFTemplateMatcher`` on the GPU, against tests/vqnnf_ref.py — the fp64
restatement that tests/test_vqnnf_cpu.py pins to the golden the reference's own code wrote — and against that golden.

Bars (all from the golden's metadata, none from what the kernels give):
  * assignment: a pixel may differ from the fp64 first minimum only where the fp64 gap between the best and the second-best
    distinct distance is below ``eps_assign`` = max(4 x the largest gap at which the reference's own fp32 assignment left
    the fp64 one, 16 fp32 ulps of the largest distance); at most 1 % of a case's pixels.  Exact ties are never set aside.
  * centroids: 4 x ``dev_centroid``, the reference's fp32 update against fp64 on the same step.
  * heat map: 4 x the case's ``dev_heat``, the reference's fp32 map against its convolutions evaluated in fp64.
  * cosine: 4 x ``dev_cosine``, fp32 torch CosineSimilarity against fp64.
Every test prints its figures before it asserts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vqnnf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

G, META = R.load_golden()
CASES = [c["name"] for c in META["cases"]]
CASE = {c["name"]: c for c in META["cases"]}
EPS = META["eps_assign"]


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tmx():
    from marie_icr_amd import template_matching

    return template_matching


def _full(img):
    return (0, 0, img.shape[1], img.shape[0])


# ---------------------------------------------------------------------------------------------------- 2. vq_assign
@pytest.mark.parametrize("name", CASES)
def test_vq_assign(ctx, tmx, name):
    window, cb = G[f"{name}/window"], G[f"{name}/cent_last"]
    got = tmx.vq_assign_host(ctx, window, _full(window), cb)
    want, gap = R.assign(R.color_features(window).reshape(27, -1).T, cb.astype(np.float64))
    ok, aside = R.codes_match(got, want, gap, EPS)
    ok_g, aside_g = R.codes_match(got, G[f"{name}/codes"], gap, EPS)
    print(f"{name}: off the fp64 first minimum {aside:.5f}, off the reference {aside_g:.5f} of the pixels; eps {EPS:.3e}; "
          f"{int((np.unique(cb, axis=0).shape[0]))} distinct of {cb.shape[0]} centroids")
    assert ok and aside <= 0.01
    assert ok_g and aside_g <= 0.01


def test_vq_assign_rectangle_wraps_around_the_window_only(ctx, tmx):
    """a rectangle of a larger image takes its neighbours from the image, and the image wraps at its own edges"""
    frame, box, cb = G["b21x33/frame"], G["b21x33/box"], G["b21x33/cent_last"]
    got = tmx.vq_assign_host(ctx, frame, box, cb)
    want, _ = R.assign(R.rect_features(frame, box), cb.astype(np.float64))
    assert np.array_equal(got.reshape(-1), want)
    edge = (0, 0, frame.shape[1], 1)                       # the top row: its upper neighbours are the bottom row
    got = tmx.vq_assign_host(ctx, frame, edge, cb)
    assert np.array_equal(got.reshape(-1), R.assign(R.rect_features(frame, edge), cb.astype(np.float64))[0])
    dup = np.repeat(cb[:5], 2, axis=0)                     # bit-equal centroids: the lower index of each pair
    got = tmx.vq_assign_host(ctx, frame, _full(frame), dup)
    assert (got % 2 == 0).all() and len(np.unique(got)) > 1


# ---------------------------------------------------------------------------------------------------- 3. kmeans_step
@pytest.mark.parametrize("name", CASES)
def test_kmeans_step_replay(ctx, tmx, name):
    frame, box = G[f"{name}/frame"], G[f"{name}/box"]
    X = R.rect_features(frame, box)
    c0 = X[G[f"{name}/init_idx"].astype(np.int64)].astype(np.float32)
    steps = (("init", c0, G[f"{name}/cent_1"]), ("1", G[f"{name}/cent_1"], G[f"{name}/cent_2"]),
             ("last-1", G[f"{name}/cent_before_last"], G[f"{name}/cent_last"]))
    for tag, src, dst in steps:
        labels, new, counts, err = tmx.vq_kmeans_step_host(ctx, frame, box, src)
        l64, c64, e64, gap = R.kmeans_step(X, src.astype(np.float64))
        ok, aside = R.codes_match(labels, l64, gap, EPS)
        dev = float(np.abs(new - dst).max())
        print(f"{name} step {tag}: labels off {aside:.5f}; centroids {dev:.3e} from the reference, "
              f"{np.abs(new - c64).max():.3e} from fp64 (bar {4 * META['dev_centroid']:.3e}); error {err:.6e} vs {e64:.6e}; "
              f"{int((counts == 0).sum())} empty")
        assert ok and aside <= 0.01
        assert dev <= 4 * META["dev_centroid"]
        assert np.array_equal(counts == 0, ~dst.any(axis=1)) and not new[counts == 0].any()
        assert np.array_equal(counts, np.bincount(labels, minlength=len(counts)))
        # the error is summed from fp32 centroids: a term (c - c0)^2 carries 2 |c - c0| 2^-24 of the centroid's rounding,
        # 1e-5 of the term at |c - c0| = 0.01; terms below that add less than 27 K 2^-24 0.01 = 2e-6 ... in all under 1e-4 of
        # an error that continues the loop, and under 1e-9 in absolute terms of one that stops it
        assert err == pytest.approx(e64, rel=1e-4, abs=1e-9)
        if tag == "last-1":
            ok, aside = R.codes_match(labels, G[f"{name}/labels"], gap, EPS)
            assert ok and aside <= 0.01
            assert err <= 1e-4 or CASE[name]["n_iter"] == 25
        else:
            assert err > 1e-4
        again = tmx.vq_kmeans_step_host(ctx, frame, box, src)
        assert np.array_equal(again[0], labels) and again[1].tobytes() == new.tobytes() and again[3] == err


@pytest.mark.parametrize("name", CASES)
def test_kmeans_loop(ctx, tmx, name):
    """the driver loop from the reference's initial draw: stops at the reference's iteration, returns the labels of the
    last assignment and the updated codebook, and two runs are bit-identical"""
    frame, box = G[f"{name}/frame"], G[f"{name}/box"]
    t = tmx.VQTemplate(ctx, frame, box, G[f"{name}/init_idx"])
    u = tmx.VQTemplate(ctx, frame, box, G[f"{name}/init_idx"])
    try:
        print(f"{name}: {t.iterations} iterations (reference {CASE[name]['n_iter']}), codebook "
              f"{np.abs(t.codebook - G[f'{name}/cent_last']).max():.3e} from the reference")
        assert t.iterations == CASE[name]["n_iter"] and t.n_codes == CASE[name]["n_code"]
        _, gap = R.assign(R.rect_features(frame, box), G[f"{name}/cent_before_last"].astype(np.float64))
        ok, aside = R.codes_match(t.labels, G[f"{name}/labels"], gap, EPS)
        assert ok and aside <= 0.01
        assert np.abs(t.codebook - G[f"{name}/cent_last"]).max() <= 4 * META["dev_centroid"]
        assert t.codebook.tobytes() == u.codebook.tobytes() and np.array_equal(t.labels, u.labels)
        if np.array_equal(t.labels, G[f"{name}/labels"]):
            gold = G[f"{name}/tmpl"]
            assert np.abs(t.responses - gold).max() <= CASE[name]["dev_tmpl"] + 2.0 ** -24 * np.abs(gold).max()
    finally:
        t.close()
        u.close()


# ---------------------------------------------------------------------------------------------------- 4. vq_heatmap
@pytest.mark.parametrize("name", CASES)
def test_vq_heatmap(ctx, tmx, name):
    codes, K, tmpl = G[f"{name}/codes"], CASE[name]["n_code"], G[f"{name}/tmpl"]
    taps, dil, wgt = G[f"{name}/taps"], G[f"{name}/dil"], G[f"{name}/wgt"]
    heat, mins = tmx.vq_heatmap_host(ctx, codes, K, tmpl, taps, dil, wgt)
    want, want_mins = R.heatmap(codes, K, tmpl, taps, dil, wgt)
    bar = 4 * CASE[name]["dev_heat"]
    print(f"{name}: max |heat - fp64| {np.abs(heat - want).max():.3e} (bar {bar:.3e}), from the reference "
          f"{np.abs(heat - G[f'{name}/heat']).max():.3e}; minima off by {np.abs(mins - want_mins).max():.3e}; "
          f"heat in [{want.min():.4f}, {want.max():.4f}]")
    assert np.abs(heat - want).max() <= bar
    assert np.abs(mins - want_mins).max() <= bar
    # the border every filter pads is the sum of the filters' minima; where only the larger filters pad, theirs
    H, W = codes.shape
    top, left = min((H - (H - 3 * d[0])) // 2 for d in dil), min((W - (W - 3 * d[1])) // 2 for d in dil)
    assert top >= 1 and left >= 1
    border = np.ones((H, W), bool)
    border[top:H - top, left:W - left] = False
    assert np.abs(heat[border] - np.float32(mins.sum())).max() <= np.spacing(np.float32(abs(mins.sum())))
    again, _ = tmx.vq_heatmap_host(ctx, codes, K, tmpl, taps, dil, wgt)
    assert again.tobytes() == heat.tobytes()


def test_vq_heatmap_large_footprint(ctx, tmx):
    """A template nearly as large as the production window: the footprint of a tile (316 x 128 cells, 121 KB) needs more
    than the 64 KiB of LDS a kernel gets by default, and the window spans several tiles in both directions.  There is no
    golden at this size: the kernel accumulates in fp64 and rounds once, so the bar is one fp32 ulp of the largest value."""
    rng = np.random.default_rng(9)
    H, W, K = 384, 128, 24
    codes = rng.integers(0, K, (H, W)).astype(np.uint8)
    codes[100:300, 20:90] = 3                                 # a large flat area: counts far above 255
    taps, dil, ker, wgt = R.filter_bank(300, 99)
    tmpl = R.template_responses(codes[40:340, 10:109], K, taps, dil, ker).astype(np.float32)
    heat, mins = tmx.vq_heatmap_host(ctx, codes, K, tmpl, taps, dil, wgt)
    want, want_mins = R.heatmap(codes, K, tmpl, taps, dil, wgt)
    bar = float(np.spacing(np.float32(np.abs(want).max())))
    print(f"large footprint: max |heat - fp64| {np.abs(heat - want).max():.3e} (bar {bar:.3e}); peak at "
          f"{np.unravel_index(np.argmax(heat), heat.shape)}")
    assert np.abs(heat - want).max() <= bar and np.abs(mins - want_mins).max() <= bar
    assert np.unravel_index(np.argmax(heat), heat.shape) == np.unravel_index(np.argmax(want), want.shape)


def test_vq_heatmap_refuses_bad_filters(ctx, tmx):
    from marie_icr_amd._lib import MarieHipError

    codes, K, tmpl = G["b9x11/codes"], CASE["b9x11"]["n_code"], G["b9x11/tmpl"]
    taps, dil, wgt = G["b9x11/taps"], G["b9x11/dil"].copy(), G["b9x11/wgt"]
    dil[0] = (0, 3)
    with pytest.raises(MarieHipError):
        tmx.vq_heatmap_host(ctx, codes, K, tmpl, taps, dil, wgt)
    dil[0] = (30, 3)                                          # a 91-row kernel on a 61-row window
    with pytest.raises(MarieHipError):
        tmx.vq_heatmap_host(ctx, codes, K, tmpl, taps, dil, wgt)
    with pytest.raises(ValueError):                            # a side below 9, before any launch
        tmx.VQTemplate(ctx, G["b9x11/frame"], (3, 3, 8, 30), np.zeros(128, np.int32))


# ---------------------------------------------------------------------------------------------------- 5. vq_peaks
def test_vq_peaks_golden(ctx, tmx):
    for win in ("a", "b"):
        names = [n for n in CASES if n.startswith(win)]
        heat = np.stack([G[f"{n}/heat"] for n in names])
        wh = [G[f"{n}/box"][2:] for n in names]
        peaks, after = tmx.vq_peaks_host(ctx, heat, wh, META["max_objects"])
        for i, n in enumerate(names):
            got = [(int(r), int(c)) for r, c, _ in peaks[i]]
            boxes = [tmx.peak_box(r, c, int(wh[i][0]), int(wh[i][1])) for r, c in got]
            print(n, "peaks", got, "boxes", boxes)
            assert got == [tuple(p) for p in G[f"{n}/peaks"].tolist()]
            assert boxes == [tuple(b) for b in G[f"{n}/boxes"].tolist()]
            want = R.peaks(G[f"{n}/heat"], int(wh[i][0]), int(wh[i][1]), META["max_objects"])
            assert [float(np.float32(v)) for _, _, v, _ in want] == [float(v) for v in peaks[i, :, 2]]
            ref_map = G[f"{n}/heat"].copy()
            for _, _, _, (x, y, w, h) in want:
                ref_map[y:y + h, x:x + w] = np.float32(R.SUPPRESSED)
            assert np.array_equal(after[i], ref_map)


def test_vq_peaks_ties_and_negative_starts(ctx, tmx):
    H, W = 23, 37
    flat = np.full((H, W), -1.0, np.float32)
    two = flat.copy()
    two[7, 30] = two[7, 5] = two[15, 2] = -0.25             # equal maxima: the first in row-major order
    corner = flat.copy()
    corner[0, 1] = 0.5                                      # a start of -3 rows: slice(-3, 5) of 23 rows is empty
    corner[20, 36] = 0.25                                   # clipped at the far edges
    all_equal = flat.copy()
    far = flat.copy()
    far[20, 36] = 0.25                                      # rows 19..23 and columns 34..39 clip at 23 and 37
    maps, wh = np.stack([two, corner, all_equal, corner, far]), [(6, 5), (5, 8), (4, 4), (9, 3), (6, 5)]
    peaks, after = tmx.vq_peaks_host(ctx, maps, wh, 3)
    for i in range(len(maps)):
        want = R.peaks(maps[i], wh[i][0], wh[i][1], 3)
        ref_map = maps[i].copy()
        for _, _, _, (x, y, w, h) in want:
            ref_map[y:y + h, x:x + w] = np.float32(R.SUPPRESSED)
        print(i, [(int(r), int(c), float(v)) for r, c, v in peaks[i]], [(r, c, v) for r, c, v, _ in want])
        assert [(int(r), int(c), float(v)) for r, c, v in peaks[i]] == [(r, c, float(np.float32(v))) for r, c, v, _ in want]
        assert np.array_equal(after[i], ref_map)
    assert [(int(r), int(c)) for r, c, _ in peaks[0]] == [(7, 5), (7, 30), (15, 2)]
    assert (int(peaks[1, 0, 0]), int(peaks[1, 1, 0])) == (0, 0) and peaks[1, 0, 2] == peaks[1, 1, 2] == 0.5   # nothing suppressed


# ---------------------------------------------------------------------------------------------------- 6. clip_cosine
def test_clip_cosine(ctx, tmx):
    pairs = R.clip_pairs(G["a36x20/window"])
    got = tmx.clip_cosine_host(ctx, np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]))
    want = np.array([R.clip_cosine(a, b) for a, b in pairs])
    bar = 4 * META["dev_cosine"]
    print("cosine", got.tolist(), "fp64", want.tolist(), "bar", bar)
    assert np.abs(got - want).max() <= bar
    assert got[0] == 1.0 and got[3] == 1.0
    black = np.zeros((1, 8, 8, 3), np.uint8)
    assert tmx.clip_cosine_host(ctx, black, black + 7)[0] == 0.0


# ---------------------------------------------------------------------------------------------------- 7. end to end
def _page():
    """a 200 x 300 page of light texture with two templates planted twice each; template frames are 96 x 128 windows"""
    rng = np.random.default_rng(77)
    page = rng.integers(236, 256, (200, 300, 3)).astype(np.uint8)
    stamps = {"alpha": rng.integers(0, 200, (36, 20, 3)).astype(np.uint8),
              "beta": rng.integers(0, 200, (20, 36, 3)).astype(np.uint8)}
    planted = {"alpha": [(40, 30), (222, 120)], "beta": [(150, 20), (60, 150)]}         # x, y
    for label, spots in planted.items():
        h, w = stamps[label].shape[:2]
        for x, y in spots:
            page[y:y + h, x:x + w] = stamps[label]
    frames, boxes, labels = [], [], []
    for label, at in (("alpha", (50, 20)), ("beta", (60, 40))):
        h, w = stamps[label].shape[:2]
        frame = rng.integers(236, 256, (96, 128, 3)).astype(np.uint8)
        frame[at[1]:at[1] + h, at[0]:at[0] + w] = stamps[label]
        frames.append(frame)
        boxes.append((at[0], at[1], w, h))
        labels.append(label)
    return page, frames, boxes, labels, planted, stamps


def ink_embedding(clip):
    """Stands in for the snippet embedding the reference takes from CLIP: the clip's ink (255 - pixel).  The feature
    similarity alone cannot tell snippets apart — small snippets are framed on a white 224 x 224 canvas, which dominates
    the cosine — and the reference leaves that to the embedding (weight 0.95)."""
    return 255.0 - clip.astype(np.float64).reshape(-1)


def test_matcher_end_to_end(ctx, tmx):
    page, frames, boxes, labels, planted, stamps = _page()
    m = tmx.VQNNFTemplateMatcher("vqnnf", ctx=ctx, seed=5, embeddings_processor=ink_embedding)
    try:
        out = m.run([page, page], frames, boxes, labels, window_size=(96, 128), max_objects=2, score_threshold=0.9)
        assert m.template_builds == 2
        for frame_idx in (0, 1):
            got = sorted((r.label, tuple(r.bbox)) for r in out if r.frame_index == frame_idx)
            want = sorted((label, (x, y, stamps[label].shape[1], stamps[label].shape[0]))
                          for label, spots in planted.items() for x, y in spots)
            print(frame_idx, got, [round(r.score, 4) for r in out if r.frame_index == frame_idx])
            assert got == want
        assert all(r.score > 0.9 and r.similarity == r.score for r in out) and len(out) == 8
        again = m.run([page], frames, boxes, labels, window_size=(96, 128), max_objects=2, score_threshold=0.9)
        assert m.template_builds == 2                          # the cached template state: no k-means launch
        assert [(r.label, r.bbox, r.score) for r in again] == [(r.label, r.bbox, r.score) for r in out if r.frame_index == 0]
        # three windows x two templates in one call against six single calls
        windows = [(0, 0, 128, 96), (102, 0, 128, 96), (172, 104, 128, 96)]
        batched = m.match_windows(page, windows, frames, boxes, 2)
        assert batched.shape == (3, 2, 2, 3)
        for wi, w in enumerate(windows):
            for ti in range(2):
                single = m.match_windows(page, [w], [frames[ti]], [boxes[ti]], 2)
                assert single.tobytes() == batched[wi, ti][None, None].tobytes()
        # a window of the page equals the same pixels as a page of their own (the neighbourhood wraps around the window)
        x, y, w, h = windows[1]
        alone = m.match_windows(np.ascontiguousarray(page[y:y + h, x:x + w]), [(0, 0, w, h)], frames, boxes, 2)
        assert alone.tobytes() == batched[1][None].tobytes()
        assert m.score(stamps["alpha"], stamps["alpha"], "weighted") == pytest.approx(1.0, abs=1e-9)
        assert m.score(stamps["alpha"], 255 - stamps["alpha"], "weighted") < 0.9
    finally:
        m.close()
