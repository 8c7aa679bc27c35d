"""CPU checks of the VQ-NNF template matcher: tests/vqnnf_ref.py (the fp64 restatement the GPU tests compare against) is
pinned to tests/golden/vqnnf.npz, which the reference's own code wrote (tools/gen_vqnnf_golden.py), and the host side of
marie_icr_amd/template_matching.py — filter bank, template responses, box arithmetic, slicing, merging, ``run`` — is
checked on the golden and on designed cases.

Tolerances: the golden's metadata records how far the reference's fp32 results are from an fp64 evaluation of the same
step (``dev_*``); the restatement is that fp64 evaluation up to float64 rounding, for which ``SLACK`` (1e-9, six orders
above float64 rounding at these magnitudes and two below the smallest recorded deviation) is added.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vqnnf_ref as R  # noqa: E402

from marie_icr_amd import template_matching as tmx  # noqa: E402
from marie_icr_amd._lib import MarieHipError  # noqa: E402

SLACK = 1e-9
G, META = R.load_golden()
CASES = [c["name"] for c in META["cases"]]
CASE = {c["name"]: c for c in META["cases"]}


def test_golden_covers_the_cases():
    shapes = {(G[f"{n}/window"].shape[:2], tuple(G[f"{n}/box"][2:])) for n in CASES}
    for win in ((96, 128), (61, 83)):
        for wh in ((20, 36), (11, 9), (33, 21)):
            assert (win, wh) in shapes
    assert all(G[f"{n}/frame"].shape == G[f"{n}/window"].shape for n in CASES)
    assert CASE["a9x11"]["n_code"] == 99 and CASE["a36x20"]["n_code"] == 128
    assert META["eps_assign"] >= 16 * np.spacing(np.float32(META["max_distance"]))
    assert os.path.getsize(R.GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", CASES)
def test_kmeans_restatement(name):
    frame, box = G[f"{name}/frame"], G[f"{name}/box"]
    X = R.rect_features(frame, box)
    labels, cent, n_iter, trail = R.kmeans_fit(X, G[f"{name}/init_idx"])
    assert n_iter == CASE[name]["n_iter"]
    _, gap = R.assign(X, G[f"{name}/cent_before_last"].astype(np.float64))
    ok, aside = R.codes_match(labels, G[f"{name}/labels"], gap, META["eps_assign"])
    assert ok and aside <= 0.01
    # equal labels at every step give the means of equal members: a step's centroids differ by that step's rounding
    for got, key in ((trail[0], "cent_1"), (trail[1], "cent_2"), (trail[-2], "cent_before_last")):
        assert np.abs(got - G[f"{name}/{key}"]).max() <= META["dev_centroid"] + SLACK
    assert np.abs(cent - G[f"{name}/cent_last"]).max() <= META["dev_fit"] + SLACK
    # one step from the reference's own centroids, empty clusters included
    for src, dst in (("cent_1", "cent_2"), ("cent_before_last", "cent_last")):
        _, new, _, _ = R.kmeans_step(X, G[f"{name}/{src}"].astype(np.float64))
        assert np.abs(new - G[f"{name}/{dst}"]).max() <= META["dev_centroid"] + SLACK
        assert np.array_equal(~new.any(axis=1), ~G[f"{name}/{dst}"].any(axis=1))


@pytest.mark.parametrize("name", CASES)
def test_query_restatement(name):
    window, box, K = G[f"{name}/window"], G[f"{name}/box"], CASE[name]["n_code"]
    feats = R.color_features(window).reshape(27, -1).T
    codes, gap = R.assign(feats, G[f"{name}/cent_last"].astype(np.float64))
    ok, aside = R.codes_match(codes, G[f"{name}/codes"], gap, META["eps_assign"])
    assert ok and aside <= 0.01
    taps, dil, ker, wgt = R.filter_bank(int(box[3]), int(box[2]))
    assert np.array_equal(taps, G[f"{name}/taps"]) and np.array_equal(dil, G[f"{name}/dil"])
    assert np.array_equal(ker, G[f"{name}/ker"]) and np.abs(wgt - G[f"{name}/wgt"]).max() <= 1e-15
    labels = G[f"{name}/labels"].reshape(int(box[3]), int(box[2]))
    tmpl = R.template_responses(labels, K, taps, dil, ker)
    assert np.abs(tmpl - G[f"{name}/tmpl"]).max() <= CASE[name]["dev_tmpl"] + SLACK
    heat, mins = R.heatmap(G[f"{name}/codes"], K, tmpl, taps, dil, wgt)
    assert np.abs(heat - G[f"{name}/heat"]).max() <= CASE[name]["dev_heat"] + SLACK
    assert heat[0, 0] == pytest.approx(mins.sum(), abs=1e-12)          # the corner is padding for every filter
    pk = R.peaks(G[f"{name}/heat"], int(box[2]), int(box[3]), META["max_objects"])
    assert [(r, c) for r, c, _, _ in pk] == [tuple(p) for p in G[f"{name}/peaks"].tolist()]
    assert [b for _, _, _, b in pk] == [tuple(b) for b in G[f"{name}/boxes"].tolist()]


def test_cosine_restatement():
    pairs = R.clip_pairs(G["a36x20/window"])
    got = [R.clip_cosine(a, b) for a, b in pairs]
    assert got[0] == pytest.approx(1.0, abs=1e-12) and got[3] == pytest.approx(1.0, abs=1e-12)
    assert 0.0 < got[2] < got[1] < 1.0
    # the features are nine permutations of the pixels, applied to both clips alike: the cosine is that of the pixels
    a, b = (p.astype(np.float32) / np.float32(255) for p in pairs[1])
    a, b = a.astype(np.float64).reshape(-1), b.astype(np.float64).reshape(-1)
    assert got[1] == pytest.approx(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)), abs=1e-12)
    assert R.clip_cosine(np.zeros((4, 4, 3), np.uint8), np.full((4, 4, 3), 9, np.uint8)) == 0.0


# ---------------------------------------------------------------------------------------------------- product, host side
@pytest.mark.parametrize("name", CASES)
def test_product_filters_and_boxes(name):
    box, K = G[f"{name}/box"], CASE[name]["n_code"]
    taps, dil, ker, wgt = tmx.filter_bank(int(box[3]), int(box[2]))
    assert np.array_equal(taps, G[f"{name}/taps"]) and np.array_equal(dil, G[f"{name}/dil"])
    assert np.array_equal(ker, G[f"{name}/ker"]) and np.abs(wgt - G[f"{name}/wgt"]).max() <= 1e-15
    tmpl = tmx.template_responses(G[f"{name}/labels"].reshape(int(box[3]), int(box[2])), K, taps, dil, ker)
    assert tmpl.dtype == np.float32
    gold = G[f"{name}/tmpl"]
    assert np.abs(tmpl - gold).max() <= CASE[name]["dev_tmpl"] + 2.0 ** -24 * np.abs(gold).max()     # + the fp32 rounding
    for (r, c), want in zip(G[f"{name}/peaks"].tolist(), G[f"{name}/boxes"].tolist()):
        assert tmx.peak_box(r, c, int(box[2]), int(box[3])) == tuple(want)
    assert tmx.n_code_of(int(box[2]), int(box[3])) == K
    idx = tmx.draw_init_indices(3, box)
    assert idx.shape == (K,) and idx.min() >= 0 and idx.max() < int(box[2]) * int(box[3])
    assert np.array_equal(idx, tmx.draw_init_indices(3, box))


def test_small_template_is_refused():
    for rows, cols in ((8, 20), (20, 8)):
        with pytest.raises(ValueError):
            tmx.filter_bank(rows, cols)
    tmx.filter_bank(9, 9)


def test_slice_image():
    s = tmx.slice_image(300, 200, 128, 96, 0.2, 0.2)          # overlap 25 rows, 19 columns
    assert s[0] == (0, 0, 96, 128) and s[1] == (77, 0, 96, 128)
    assert s[2] == (104, 0, 96, 128)                          # 154 + 96 overruns 200: moved back to 200 - 96
    assert all(x >= 0 and y >= 0 and x + w <= 200 and y + h <= 300 and (w, h) == (96, 128) for x, y, w, h in s)
    assert sorted({y for _, y, _, _ in s}) == [0, 103, 172]   # 206 + 128 overruns 300: moved back to 172
    covered = np.zeros((300, 200), bool)
    for x, y, w, h in s:
        covered[y:y + h, x:x + w] = True
    assert covered.all()
    assert tmx.slice_image(128, 96, 128, 96) == [(0, 0, 96, 128)]
    assert tmx.slice_image(100, 50, 128, 96) == [(0, 0, 50, 100)]     # a page smaller than the slice: the page
    # the default production geometry: a 2550 x 3300 page in 384 x 128 windows
    big = tmx.slice_image(3300, 2550, 384, 128)
    assert len(big) == 11 * 25 and len(set(big)) == len(big)


def _pred(x0, y0, x1, y1, score, label):
    return tmx.ObjectPrediction([x0, y0, x1, y1], score, label)


def test_greedy_nmm():
    nmm = tmx.GreedyNMMPostprocess(match_threshold=0.5, match_metric="IOS", class_agnostic=False)
    # two overlapping boxes of one label: the union, the higher score
    out = nmm([_pred(0, 0, 10, 10, 0.91, "a"), _pred(4, 0, 14, 10, 0.97, "a")])
    assert len(out) == 1 and out[0].bbox == [0, 0, 14, 10] and out[0].score == 0.97 and out[0].category == "a"
    # different labels do not merge
    out = nmm([_pred(0, 0, 10, 10, 0.91, "a"), _pred(4, 0, 14, 10, 0.97, "b")])
    assert sorted(p.category for p in out) == ["a", "b"] and sorted(p.bbox for p in out) == [[0, 0, 10, 10], [4, 0, 14, 10]]
    # intersection over the smaller area just under and just over 0.5: 49 and 51 of the 100 pixels of the smaller box
    assert tmx.box_ios([0, 0, 100, 1], [51, 0, 151, 1]) == pytest.approx(0.49)
    assert len(nmm([_pred(0, 0, 100, 1, 0.95, "a"), _pred(51, 0, 151, 1, 0.93, "a")])) == 2
    assert tmx.box_ios([0, 0, 100, 1], [49, 0, 149, 1]) == pytest.approx(0.51)
    over = nmm([_pred(0, 0, 100, 1, 0.95, "a"), _pred(49, 0, 149, 1, 0.93, "a")])
    assert len(over) == 1 and over[0].bbox == [0, 0, 149, 1] and over[0].score == 0.95
    # a small box inside a large one merges whatever their IoU; the highest score leads
    out = nmm([_pred(2, 2, 6, 6, 0.92, "a"), _pred(0, 0, 100, 100, 0.99, "a"), _pred(200, 0, 210, 10, 0.95, "a")])
    assert [p.bbox for p in out] == [[0, 0, 100, 100], [200, 0, 210, 10]] and [p.score for p in out] == [0.99, 0.95]
    assert tmx.GreedyNMMPostprocess(class_agnostic=True)([_pred(0, 0, 10, 10, 0.9, "a"), _pred(1, 0, 11, 10, 0.8, "b")])[0].category == "a"


def test_extract_windows():
    image = np.arange(200 * 300 * 3, dtype=np.uint32).reshape(200, 300, 3).astype(np.uint8)
    wins, boxes = tmx.BaseTemplateMatcher.extract_windows(image, [(140, 90, 20, 10), (2, 3, 20, 10), (290, 195, 10, 5)],
                                                          (64, 96))
    assert all(w.shape == (64, 96, 3) for w in wins)
    assert boxes[0] == (38, 27, 20, 10) and np.array_equal(wins[0], image[63:127, 102:198])
    assert boxes[1] == (2, 3, 20, 10) and np.array_equal(wins[1], image[:64, :96])              # clamped at the origin
    assert boxes[2] == (86, 59, 10, 5) and np.array_equal(wins[2], image[136:, 204:])           # moved back inside
    for (x, y, w, h), win, src in zip(boxes, wins, [(140, 90, 20, 10), (2, 3, 20, 10), (290, 195, 10, 5)]):
        assert np.array_equal(win[y:y + h, x:x + w], image[src[1]:src[1] + src[3], src[0]:src[0] + src[2]])
    with pytest.raises(ValueError):
        tmx.BaseTemplateMatcher.extract_windows(image[:50], [(1, 1, 5, 5)], (64, 96))
    wins, boxes = tmx.BaseTemplateMatcher.extract_windows(image[:50], [(1, 1, 5, 5)], (64, 96), allow_padding=True)
    assert wins[0].shape == (64, 96, 3) and (wins[0][50:] == 255).all() and boxes[0] == (1, 1, 5, 5)


class StubMatcher(tmx.BaseTemplateMatcher):
    """predicts, in every window, the boxes planted for it (window-relative), and records what it was asked"""

    def __init__(self, planted, slicing_enabled=True):
        super().__init__(slicing_enabled)
        self.planted, self.calls = planted, []

    def predict(self, frame, template_frames, template_boxes, template_labels, template_texts=None, score_threshold=0.9,
                scoring_strategy="weighted", max_objects=1, batch_size=1, words=None, word_boxes=None, word_lines=None):
        self.calls.append(frame.shape[:2])
        return [tmx.TemplateMatchResult(bbox=b, label=lab, score=s, similarity=s, frame_index=-1)
                for b, lab, s in self.planted.get(len(self.calls) - 1, [])]


def _run(m, frames, window=(64, 96), **kw):
    tf = [np.zeros(window + (3,), np.uint8)]
    return m.run(frames, tf, [(1, 1, 20, 10)], ["t"], window_size=window, **kw)


def test_run_on_a_stub_matcher():
    frame = np.zeros((100, 150, 3), np.uint8)
    windows = tmx.slice_image(100, 150, 64, 96)
    assert windows == [(0, 0, 96, 64), (54, 0, 96, 64), (0, 36, 96, 64), (54, 36, 96, 64)]
    planted = {0: [((10, 5, 20, 10), "a", 0.95)],
               1: [((0, 6, 20, 10), "a", 0.99), ((60, 40, 8, 8), "b", 0.9)],       # 0.9 is not above the threshold
               3: [((30, 0, 12, 6), "b", 0.93)]}
    m = StubMatcher(planted)
    out = _run(m, [frame, frame], score_threshold=0.9)
    assert m.calls[:4] == [(64, 96)] * 4 and len(m.calls) == 8
    first = [r for r in out if r.frame_index == 0]
    # window 1's box shifts by (54, 0) -> (54, 6, 20, 10), disjoint from window 0's; labels grouped in score order
    assert [(r.bbox, r.label, r.score) for r in first] == [([54, 6, 20, 10], "a", 0.99), ([10, 5, 20, 10], "a", 0.95),
                                                           ([84, 36, 12, 6], "b", 0.93)]
    assert all(r.similarity == r.score for r in out) and [r for r in out if r.frame_index == 1] == []
    # overlapping predictions of neighbouring windows merge
    m = StubMatcher({0: [((60, 5, 20, 10), "a", 0.95)], 1: [((8, 5, 20, 10), "a", 0.97)]})
    out = _run(m, [frame])
    assert [(r.bbox, r.score) for r in out] == [([60, 5, 22, 10], 0.97)]
    assert _run(StubMatcher({}, slicing_enabled=False), [frame]) == []
    m = StubMatcher({}, slicing_enabled=False)
    _run(m, [frame])
    assert m.calls == [(100, 150)]


def test_filter_scores_is_strict():
    m = StubMatcher({})
    b, l, s = m.filter_scores([[0, 0, 1, 1], [1, 1, 2, 2], [2, 2, 3, 3]], ["a", "b", "c"], [0.9, 0.9000001, 0.5],
                              [None] * 3, 0.9)
    assert (b, l, s) == ([[1, 1, 2, 2]], ["b"], [0.9000001])


@pytest.mark.parametrize("kw", [{"score_threshold": 1.5}, {"score_threshold": -0.1}, {"max_overlap": 2}, {"max_objects": 0},
                                {"downscale_factor": 1.5}, {"downscale_factor": -1}, {"batch_size": 0},
                                {"regions": [(0, 0, 1, 1), (0, 0, 1, 1)]}])
def test_run_validations(kw):
    with pytest.raises(ValueError):
        _run(StubMatcher({}), [np.zeros((100, 150, 3), np.uint8)], **kw)


def test_run_refuses_what_is_not_built():
    frame = np.zeros((100, 150, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        _run(StubMatcher({}), [frame], downscale_factor=0.5)
    with pytest.raises(ValueError):      # a template frame of another size than the window
        StubMatcher({}).run([frame], [np.zeros((64, 90, 3), np.uint8)], [(1, 1, 20, 10)], ["t"], window_size=(64, 96))
    with pytest.raises(NotImplementedError):
        tmx.VQNNFTemplateMatcher("m", n_feature=512)
    with pytest.raises(NotImplementedError):
        tmx.VQNNFTemplateMatcher("m", pca_dims=128)
    with pytest.raises(MarieHipError):
        tmx.VQNNFTemplateMatcher("m", use_gpu=False)


def test_composite_break_on_match():
    frame = np.zeros((100, 150, 3), np.uint8)
    empty, a, b = StubMatcher({}), StubMatcher({0: [((10, 5, 20, 10), "a", 0.95)]}), StubMatcher({0: [((12, 5, 20, 10), "a", 0.99)]})
    out = _run(tmx.CompositeTemplateMatcher([empty, a, b], break_on_match=True), [frame], score_threshold=0.8)
    assert [(r.bbox, r.score, r.frame_index) for r in out] == [([10, 5, 20, 10], 0.95, 0)] and b.calls == []
    for m in (empty, a, b):
        m.calls.clear()
    out = _run(tmx.CompositeTemplateMatcher([empty, a, b], break_on_match=False), [frame], score_threshold=0.8)
    assert [(r.bbox, r.score) for r in out] == [([10, 5, 22, 10], 0.99)] and len(b.calls) == 4      # both ran, then merged
    with pytest.raises(NotImplementedError):
        tmx.CompositeTemplateMatcher([a]).predict(frame, [], [], [])
