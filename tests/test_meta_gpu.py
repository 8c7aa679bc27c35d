"""MetaTemplateMatcher on the MI355X: the n-gram edit-distance kernel (marie_icr_amd/csrc/lev_ngrams.hip) against the textbook DP
of tests/meta_ref.py, and ``predict`` / ``score_candidates`` / ``run`` against the one-pair-at-a-time restatement there.

Bars:
  * distances and candidate lengths are integers: equal, everywhere, including the -1 of "no candidate";
  * with callable embedders the matcher and the restatement do the same double arithmetic on the same vectors: boxes, labels and
    rounded scores equal;
  * with an embeddings object the Levenshtein term is equal and the two cosines are compared with the same object called one
    item at a time (host cosine in double of its fp32 embeddings): 2 x constants measured on the MI355X, the project's
    convention for a single-seed measurement.
Every test prints its figures before it asserts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as V  # noqa: E402
import cliptext_ref as T  # noqa: E402
import meta_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# batched (one encoder call per tower, pair_cosines on the device) against the same embeddings object one item at a time with
# the cosine in double on the host, max over the fixture's six candidates at lev >= 0.5.  First MI355X run: fp32 mode text
# 1.089e-7, image 6.60e-8; f16 mode text 1.089e-7, image 1.330e-7 — the rounding of the device's fp32 cosine: the embeddings of
# a batch are those of the single calls.
COS_TEXT_ERR_MEASURED = {"f32": 1.089e-7, "f16": 1.089e-7}
COS_IMAGE_ERR_MEASURED = {"f32": 6.60e-8, "f16": 1.330e-7}
# the restated totals at lev >= 0.5 are 0.8188, 0.8472, 0.8528 | 0.9117, 0.9644, 0.9998 in both modes (to 4 digits), the others
# are below 0.5: the threshold sits in the widest gap, 0.027 from its nearest total (asserted on the restatement to be >= 0.02)
REAL_THRESHOLD = {"f32": 0.88, "f16": 0.88}

PATTERN_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 256, 257, 1024)
LETTERS = "ABCD"
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    for key in list(_cache):
        if key[0] == "emb":
            _cache.pop(key).close()
    c.close()


@pytest.fixture(scope="module")
def tmx():
    from marie_icr_amd import template_matching

    return template_matching


# ---------------------------------------------------------------------------------------------------- 1. the kernel
def _word(rng, n, letters=LETTERS):
    return "".join(rng.choice(list(letters), n))


def _mutate(rng, word):
    """one substitution, one deletion and one insertion (where the word is long enough), in lower case: upper() is the layout's"""
    w = list(word.lower())
    if len(w) > 2:
        w[len(w) // 2] = "b" if w[len(w) // 2] != "b" else "c"
        del w[0]
        w.insert(len(w) - 1, "x")
    return "".join(w)


def designed_page(m, seed):
    """A pattern of exactly ``m`` code points made of g words, and a page holding: the pattern's words themselves (a candidate
    equal to the pattern), a mutated copy, copies with blanks, tabs and no-break spaces at both ends, empty and blank words,
    words without any letter of the pattern (ids 0 only), and random words: candidates shorter than, as long as and longer
    than the pattern at the three n-gram sizes"""
    rng = np.random.default_rng(seed)
    g = 1 if m < 8 else 4
    body = m - (g - 1)
    lens = [body // g + (1 if k < body % g else 0) for k in range(g)]
    pwords = [_word(rng, n) for n in lens]
    pattern = " ".join(pwords)
    assert len(pattern) == m and len(pattern.split(" ")) == g
    typical = max(lens[0], 1)
    words = [_word(rng, typical), "xyz", "q"]
    words += [w.lower() for w in pwords]
    words += ["", " "] + [_mutate(rng, w) for w in pwords]
    words += ["\t " + pwords[0].lower()] + [w.lower() for w in pwords[1:]]
    words[-1] = words[-1] + "  "
    words += ["zz", _word(rng, typical + 3, LETTERS + "xy"), "", _word(rng, max(typical - 2, 0)), "yx" * (typical // 2 + 1)]
    return words, pattern, g


def _check_kernel(ctx, tmx, words, patterns, gs, lines=None, distance=R.dp_distance, memo=None):
    layout = tmx.text_layout(words, patterns)
    dist, length = tmx.lev_ngrams_host(ctx, layout, gs, lines)
    want_d, want_l = R.expected_tables(words, patterns, gs, lines, distance, memo)
    pairs = int((want_d >= 0).sum())
    print(f"N {len(words)} T {len(patterns)} m {[len(p) for p in patterns]} g {list(gs)} lines {lines is not None}: {pairs} pairs, "
          f"{int((want_d < 0).sum())} empty cells, distances {want_d[want_d >= 0].min() if pairs else '-'} .. "
          f"{want_d.max()}, {int((want_d == 0).sum())} equal, wrong dist {int((dist != want_d).sum())} len "
          f"{int((length != want_l).sum())}")
    assert dist.dtype == np.int32 and dist.shape == (len(patterns), 3, len(words)) == length.shape
    assert np.array_equal(length, want_l)
    assert np.array_equal(dist, want_d)
    return want_d, want_l


@pytest.mark.parametrize("m", PATTERN_LENGTHS)
def test_kernel_equals_the_dp_on_designed_pages(ctx, tmx, m):
    words, pattern, g = designed_page(m, 40 + m)
    distance = R.dp_distance if m <= 129 else R.dp_distance_rows
    memo = {}
    want_d, want_l = _check_kernel(ctx, tmx, words, [pattern], [g], None, distance, memo)
    got = want_l[want_d >= 0]
    assert (got < m).any() or m == 0
    assert (got == m).any() and (got > m).any()
    assert (want_d == 0).sum() >= 1                                     # the pattern's own words, and their copy to be stripped
    if g == 1:                                                          # "xyz": no common character, the larger length
        assert want_d[0, 1, 1] == max(3, m) and want_l[0, 1, 1] == 3
    lines = [k // 5 for k in range(len(words))]
    _check_kernel(ctx, tmx, words, [pattern], [g], lines, distance, memo)


def test_kernel_edge_sizes_and_mixed_instances(ctx, tmx):
    rng = np.random.default_rng(5)
    # N = 1, T = 1: sizes 1 (g = 1, 2) or none (g = 3)
    for g, pattern in ((1, "ABC"), (2, "AB C"), (3, "A B C")):
        want_d, _ = _check_kernel(ctx, tmx, [" abd "], [pattern], [g])
        assert (want_d >= 0).sum() == (1 if g < 3 else 0)
    # N = 65 (3 N = 195 < one tile), T = 3 with one-, two- and sixteen-word bit vectors in one call, lines present and absent
    words = [_word(rng, int(rng.integers(0, 9)), LETTERS + "x ") for _ in range(65)]
    patterns = [" ".join(_word(rng, 5) for _ in range(3)), " ".join(_word(rng, 6) for _ in range(14)),
                " ".join(_word(rng, 7) for _ in range(125))]
    assert [(len(p) + 63) // 64 for p in patterns] == [1, 2, 16]
    gs = [3, 14, 65]                             # the ABI takes g on its own; 65 + 1 > N: size g + 1 has no candidate
    lines = np.sort(rng.integers(0, 6, 65)).tolist()
    memo = {}
    for ln in (None, lines):
        want_d, _ = _check_kernel(ctx, tmx, words, patterns, gs, ln, R.dp_distance_rows, memo)
        assert (want_d[2, 2] == -1).all() and (want_d[0] >= 0).any() and ((want_d[2, :2] >= 0).sum() == 3 or ln is not None)
    # ids of 0 only: no blank in the pattern, so not even the blanks between the words match
    want_d, want_l = _check_kernel(ctx, tmx, ["xyz", "q", "zz"] * 3, ["ABCD" * 17 + "AB"], [2])
    assert np.array_equal(want_d[want_d >= 0], np.maximum(want_l[want_d >= 0], 70))
    # 3 N = 300: the tile boundary (256 candidates a workgroup) falls inside size g + 1's range, T = 3 patterns of one instance
    words = [_word(rng, int(rng.integers(1, 6)), LETTERS + "x") for _ in range(100)]
    patterns = [" ".join(words[40:42]).upper(), _word(rng, 9), "AB CD B"]
    _check_kernel(ctx, tmx, words, patterns, [2, 1, 3])


def test_kernel_random_pairs(ctx, tmx):
    """about 2,000 pairs over a 4-letter alphabet: the distances are neither 0 nor the length"""
    rng = np.random.default_rng(11)
    words = [_word(rng, int(rng.integers(2, 8))) for _ in range(230)]
    patterns = [" ".join(_word(rng, int(rng.integers(2, 8))) for _ in range(g)) for g in (2, 3, 4)]
    want_d, want_l = _check_kernel(ctx, tmx, words, patterns, [2, 3, 4], None, R.dp_distance_rows)
    ok = want_d >= 0
    assert ok.sum() >= 2000
    m = np.array([len(p) for p in patterns])[:, None, None]
    inner = ok & (want_d > 0) & (want_d < np.maximum(want_l, m))
    print(f"{int(inner.sum())} of {int(ok.sum())} distances strictly between 0 and the larger length")
    assert inner.sum() > 0.9 * ok.sum()


def test_kernel_refusals(ctx, tmx):
    from marie_icr_amd._lib import MarieHipError

    with pytest.raises(ValueError, match="1025 code points"):
        tmx.lev_ngrams_host(ctx, tmx.text_layout(["a"], ["A" * 1025]), [1])
    layout = tmx.text_layout(["ab", "c"], ["AB"])
    layout.fs[1] = 99                                                      # outside S: the library checks before it launches
    with pytest.raises(MarieHipError, match="outside"):
        tmx.lev_ngrams_host(ctx, layout, [1])
    layout = tmx.text_layout(["ab", "c"], ["AB"])
    layout.page_ids[0] = 7
    with pytest.raises(MarieHipError, match="alphabet"):
        tmx.lev_ngrams_host(ctx, layout, [1])


# ---------------------------------------------------------------------------------------------------- 2. predict, callables
def _vector(key: bytes) -> np.ndarray:
    """a seeded vector per key, with a common component: cosines around 0.98"""
    return 1.0 + 0.15 * np.random.default_rng(list(key[:48]) + [len(key)]).standard_normal(32)


class Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, x):
        self.calls += 1
        return self.fn(x)


def embed_text(text):
    return _vector(text.encode("utf-8"))


def embed_clip(clip):
    return _vector(clip[::8, ::8].tobytes())


def text_page():
    """a 96 x 256 frame with 12 words on three lines and three templates: an exact hit ("Invoice total"), a near miss with
    one edit ("amount due" against "amount duo") and an absent one"""
    rng = np.random.default_rng(21)
    frame = rng.integers(0, 256, (96, 256, 3)).astype(np.uint8)
    words = ["Invoice", "total", "net", "30", "amount", "duo", "paid", "on", "ref", " 17 ", "", "thanks"]
    boxes = [[6 + 62 * (k % 4), 8 + 30 * (k // 4), 56, 18] for k in range(12)]
    lines = [1 + k // 4 for k in range(12)]
    tframes = [rng.integers(0, 256, (48, 96, 3)).astype(np.uint8) for _ in range(3)]
    tboxes = [(4, 6, 60, 20), (-2, 10, 50, 16), (8, 8, 40, 12)]
    return frame, words, boxes, lines, tframes, tboxes, ["head", "due", "none"], ["Invoice total", "amount due", "purchase order"]


def _clip_of(ctx, tmx):
    return lambda snippet: np.ascontiguousarray(tmx.resize_image(np.ascontiguousarray(snippet), tmx.CLIP_SIZE, ctx=ctx)[0])


def test_predict_with_callable_embedders(ctx, tmx):
    frame, words, boxes, lines, tframes, tboxes, labels, texts = text_page()
    clips, txt = Counting(embed_clip), Counting(embed_text)
    m = tmx.MetaTemplateMatcher("meta", ctx=ctx, embeddings_processor=clips, text_embeddings_processor=txt)
    ref = R.Scorer(embed_text, embed_clip, _clip_of(ctx, tmx))
    for thr, ln in ((0.9, lines), (0.9, None), (0.96, lines), (0.4, lines)):
        totals = []
        want = R.predict(ref, frame, tframes, tboxes, labels, texts, thr, words, boxes, ln, totals)
        got = m.predict(frame, tframes, tboxes, labels, texts, thr, words=words, word_boxes=boxes, word_lines=ln)
        print(thr, ln is not None, [(p.label, list(p.bbox), p.score) for p in got], f"{len(totals)} pairs scored")
        assert [(list(p.bbox), p.label, p.score) for p in got] == [(list(b), l, s) for b, l, s in want]
    hits = m.predict(frame, tframes, tboxes, labels, texts, 0.9, words=words, word_boxes=boxes, word_lines=lines)
    assert [(p.label, list(p.bbox)) for p in hits] == [("head", [6, 8, 118, 18]), ("due", [6, 38, 118, 18])]
    # the caches: a second predict on the same page embeds nothing again
    before = (clips.calls, txt.calls)
    assert before[0] > 0 and before[1] > 0
    again = m.predict(frame, tframes, tboxes, labels, texts, 0.9, words=words, word_boxes=boxes, word_lines=lines)
    assert (clips.calls, txt.calls) == before and [(p.bbox, p.score) for p in again] == [(p.bbox, p.score) for p in hits]
    # score, one pair: below 0.5 the Levenshtein term alone
    assert m.score("INVOICE TOTAL", "PURCHASE ORDER", frame[8:26, 6:124], tframes[2][8:20, 8:48]) == \
        ref.score("INVOICE TOTAL", "PURCHASE ORDER", frame[8:26, 6:124], tframes[2][8:20, 8:48]) < 0.5
    assert m.score("AMOUNT DUO", "AMOUNT DUE", frame[38:56, 6:124], tframes[1][10:26, 0:50]) == \
        ref.score("AMOUNT DUO", "AMOUNT DUE", frame[38:56, 6:124], tframes[1][10:26, 0:50])
    with pytest.raises(ValueError, match="empty snippet"):
        m.predict(frame, tframes, tboxes, labels, texts, 0.9, words=words, word_boxes=[[300, 8, 10, 10]] * 12)


# ---------------------------------------------------------------------------------------------------- 3. two real towers
def _embeddings(ctx, precision, tmp_path_factory):
    from marie_icr_amd import embeddings
    from marie_icr_amd.clip_tokenizer import ClipTokenizer

    if ("emb", precision) not in _cache:
        if "tok" not in _cache:
            d = str(tmp_path_factory.mktemp("meta_vocab"))
            T.make_vocab(d)
            _cache["tok"] = (ClipTokenizer.from_dir(d),)
        both = dict(V.make_state(V.SMALL, *V.GAINS["small"], seed=0), **T.make_state(T.SMALL, seed=0))
        _cache[("emb", precision)] = embeddings.ClipImageEmbeddings(state=both, precision=precision, ctx=ctx, tokenizer=_cache["tok"][0])
    return _cache[("emb", precision)]


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_predict_with_a_two_tower_checkpoint(ctx, tmx, tmp_path_factory, precision):
    frame, words, boxes, lines, tframes, tboxes, labels, texts = text_page()
    frame = frame // 2 + np.linspace(0, 127, 256).astype(np.uint8)[None, :, None]      # the snippets differ along the page
    e = _embeddings(ctx, precision, tmp_path_factory)
    m = tmx.MetaTemplateMatcher("meta", ctx=ctx, embeddings_processor=e)
    ref = R.Scorer(lambda t: e.embed_texts([t], truncation=True)[0], lambda c: e.embed_clips(c[None])[0], _clip_of(ctx, tmx))
    thr = REAL_THRESHOLD[precision]
    totals = []
    want = R.predict(ref, frame, tframes, tboxes, labels, texts, thr, words, boxes, lines, totals)
    calls = (e.encoder_calls, e.text_encoder_calls)
    cands = m.score_candidates(frame, tframes, tboxes, texts, words, boxes, lines)
    batched = (e.encoder_calls - calls[0], e.text_encoder_calls - calls[1])
    d_text = d_image = 0.0
    for c in cands:
        x, y, w, h = c.bbox
        tx, ty, tw, th = tboxes[c.template]
        tx, ty = max(tx, 0), max(ty, 0)
        lev, cos_text, cos_image, total = ref.terms(c.words, texts[c.template].strip().upper(), frame[y:y + h, x:x + w],
                                                    tframes[c.template][ty:ty + th, tx:tx + tw])
        print(f"{precision} {labels[c.template]:5s} n {c.ngram} i {c.start:2d} {c.words!r:18s} lev {c.lev:.4f} cos_text {c.cos_text:.6f} "
              f"({c.cos_text - cos_text:+.2e}) cos_image {c.cos_image:.6f} ({c.cos_image - cos_image:+.2e}) total {c.total:.6f}")
        assert c.lev == lev and lev >= 0.5
        assert c.total == (c.lev + c.cos_text + c.cos_image) / 3
        d_text, d_image = max(d_text, abs(c.cos_text - cos_text)), max(d_image, abs(c.cos_image - cos_image))
    near = min(abs(t - thr) for t in totals)
    print(f"{precision}: {len(cands)} candidates at lev >= 0.5 of {len(totals)} pairs, encoder calls {batched}, max |d cos_text| "
          f"{d_text:.3e} |d cos_image| {d_image:.3e}; restated totals {sorted(round(t, 4) for t in totals if t >= 0.5)}, nearest to "
          f"the threshold {thr}: {near:.4f}")
    by_dp = [(t, n, i) for t, text in enumerate(texts) for _, i, n in R.candidates(len(words), len(text.split(" ")), lines)
             if 1 - R.dp_distance(R.ngram_text(words, i, n), text.upper()) / max(len(R.ngram_text(words, i, n)), len(text)) >= 0.5]
    assert [(c.template, c.ngram, c.start) for c in cands] == by_dp and len(cands) >= 4
    assert batched == (1, 1)                                               # one encoder call per tower for the whole page
    assert d_text <= 2 * COS_TEXT_ERR_MEASURED[precision]
    assert d_image <= 2 * COS_IMAGE_ERR_MEASURED[precision]
    assert near >= 0.02, "the fixture must keep every restated total away from the threshold"
    got = m.predict(frame, tframes, tboxes, labels, texts, thr, words=words, word_boxes=boxes, word_lines=lines)
    print([(p.label, list(p.bbox), p.score) for p in got])
    assert [(list(p.bbox), p.label) for p in got] == [(list(b), l) for b, l, _ in want] and len(got) >= 1
    # the caches: nothing is embedded again
    calls = (e.encoder_calls, e.text_encoder_calls, e.clips_embedded, e.texts_embedded)
    again = m.predict(frame, tframes, tboxes, labels, texts, thr, words=words, word_boxes=boxes, word_lines=lines)
    assert (e.encoder_calls, e.text_encoder_calls, e.clips_embedded, e.texts_embedded) == calls
    assert [(p.bbox, p.score) for p in again] == [(p.bbox, p.score) for p in got]


def test_a_missing_text_side_is_refused(ctx, tmx):
    from marie_icr_amd import embeddings

    e = embeddings.ClipImageEmbeddings(state=V.make_state(V.SMALL, *V.GAINS["small"], seed=0), precision="f32", ctx=ctx)
    try:
        with pytest.raises(ValueError, match="text"):
            tmx.MetaTemplateMatcher("meta", ctx=ctx, embeddings_processor=e)
        assert tmx.MetaTemplateMatcher("meta", ctx=ctx, embeddings_processor=e, text_embeddings_processor=embed_text)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 4. the composite
def test_composite_returns_the_text_hit(ctx, tmx):
    from test_vqnnf_gpu import _page, ink_embedding

    page, frames, boxes, labels, planted, stamps = _page()
    texts = ["total due", "no such text"]
    # a hand-made OCR result: nothing on page 0; on page 1 the text on clear paper, away from the planted stamps
    ocr_words = [{"text": "Total", "box": [100, 90, 30, 12], "line": 1}, {"text": "due", "box": [134, 90, 22, 12], "line": 1},
                 {"text": "other", "box": [10, 180, 30, 12], "line": 2}]
    metadata = [{"words": []}, {"words": ocr_words}]
    vq = tmx.VQNNFTemplateMatcher("vqnnf", ctx=ctx, seed=5, embeddings_processor=ink_embedding)
    meta = tmx.MetaTemplateMatcher("meta", ctx=ctx, embeddings_processor=embed_clip, text_embeddings_processor=embed_text)
    try:
        direct = meta.predict(page, frames, boxes, labels, texts, 0.9, words=[w["text"] for w in ocr_words],
                              word_boxes=[w["box"] for w in ocr_words], word_lines=[w["line"] for w in ocr_words])
        assert [(p.label, list(p.bbox)) for p in direct] == [("alpha", [100, 90, 56, 12])] and direct[0].score > 0.9
        alone = vq.run([page, page], frames, boxes, labels, window_size=(96, 128), max_objects=2, score_threshold=0.9)
        out = tmx.CompositeTemplateMatcher([vq, meta]).run([page, page], frames, boxes, labels, template_texts=texts,
                                                           metadata=metadata, window_size=(96, 128), max_objects=2,
                                                           score_threshold=0.9)
        print([(r.label, r.bbox, round(r.score, 4), r.frame_index) for r in out])
        hit = [r for r in out if list(r.bbox) == [100, 90, 56, 12]]
        assert len(hit) == 1 and (hit[0].label, hit[0].frame_index, hit[0].score) == ("alpha", 1, direct[0].score)
        rest = sorted((r.label, tuple(r.bbox), r.score, r.frame_index) for r in out if r is not hit[0])
        assert rest == sorted((r.label, tuple(r.bbox), r.score, r.frame_index) for r in alone)      # VQ-NNF ignores the words
    finally:
        vq.close()
