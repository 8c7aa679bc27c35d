"""CPU checks of MetaTemplateMatcher's host side (marie_icr_amd/template_matching.py) against tests/meta_ref.py: the
page-as-one-string layout on designed word lists, the blocked Myers recurrence of csrc/lev_ngrams.hip (restated in Python over
bit tables built from the product's layout) against the textbook DP, the n-gram enumeration at its edges, acceptance and
overlap suppression of ``predict`` (with the kernel's tables supplied by the DP), ``BaseTemplateMatcher.run`` handing a page's
words to ``predict``, and the refusals that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_ref as R  # noqa: E402

from marie_icr_amd import template_matching as tmx  # noqa: E402
from marie_icr_amd._lib import MarieHipError  # noqa: E402

ASTRAL = "\U0001F600"
# empty words, leading / trailing blanks, tabs, no-break spaces, a letter whose upper() lengthens it, astral code points, words of
# white space only at both ends and in the middle
WORD_LISTS = [
    ["Invoice", "total", "due"],
    ["", "ab", "", "", "cd", ""],
    [" lead", "trail ", " both ", "\ttab\t", "\u00a0nbsp\u00a0"],
    ["stra\u00dfe", "\u00df", "\u01f0", "\ufb01n"],
    [ASTRAL + "x", "y" + ASTRAL, ASTRAL],
    [" ", "\t", "x", "\u00a0", " "],
    ["", "", ""],
    ["a b", " c  d ", "e"],
    ["x"],
]
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200)


@pytest.mark.parametrize("words", WORD_LISTS, ids=range(len(WORD_LISTS)))
def test_layout_spans_are_the_reference_strings(words):
    patterns = ["STRASSE", "AB CD", ASTRAL + "X"]
    lay, ref = tmx.text_layout(words, patterns), R.layout(words, patterns)
    assert lay.text == ref["S"] == " ".join(words).upper()
    for name in ("ws", "we", "fs", "le"):
        assert getattr(lay, name).tolist() == ref[name], name
    assert lay.page_ids.tolist() == ref["page_ids"] and lay.alphabet == len(ref["letters"])
    assert lay.pattern_ids.tolist() == [c for p in ref["pattern_ids"] for c in p]
    assert lay.pattern_off.tolist() == [0, 7, 12, 14]
    assert len(lay.page_ids) == len(lay.text)                       # code points, not UTF-16 units
    for i in range(len(words)):
        for n in range(1, len(words) - i + 1):
            a, b = lay.span(i, n)
            assert lay.text[a:b] == R.ngram_text(words, i, n), (i, n)
            assert (a, b) == R.span(ref, i, n)


def test_layout_ids():
    lay = tmx.text_layout(["abc", "Zed", ASTRAL], ["CAB", ASTRAL + "E"])
    # alphabet: sorted code points of the patterns A B C E astral -> 1 .. 5; blanks, Z and D are outside it
    assert lay.alphabet == 5
    assert lay.page_ids.tolist() == [1, 2, 3, 0, 0, 4, 0, 0, 5]
    assert lay.pattern_ids.tolist() == [3, 1, 2, 5, 4]
    empty = tmx.text_layout(["ab"], [""])
    assert empty.alphabet == 0 and empty.page_ids.tolist() == [0, 0] and empty.pattern_off.tolist() == [0, 0]


def test_dp_distance():
    assert R.dp_distance("kitten", "sitting") == 3 and R.dp_distance("", "abc") == 3 and R.dp_distance("abc", "") == 3
    assert R.dp_distance("flaw", "lawn") == 2 and R.dp_distance("same", "same") == 0 and R.dp_distance("", "") == 0


def test_dp_by_rows_equals_the_dp():
    rng = np.random.default_rng(9)
    for la, lb in ((0, 0), (0, 5), (5, 0), (1, 1), (7, 9), (40, 33), (64, 65), (130, 120)):
        for letters in ("AB", "ABCD" + ASTRAL):
            a, b = "".join(rng.choice(list(letters), la)), "".join(rng.choice(list(letters), lb))
            assert R.dp_distance_rows(a, b) == R.dp_distance(a, b)
            assert R.dp_distance_rows(a, a) == 0


@pytest.mark.parametrize("m", LENGTHS)
def test_blocked_myers_equals_the_dp(m):
    """the recurrence of csrc/lev_ngrams.hip over bit tables built from the product's ids; text lengths 0 .. 300, with
    characters outside the pattern's alphabet (id 0)"""
    rng = np.random.default_rng(100 + m)
    letters = "ABCD"
    pattern = "".join(rng.choice(list(letters), m))
    texts = []
    for n in (0, 1, 2, 5, 62, 63, 64, 65, 66, 127, 128, 129, 199, 200, 201, 300, max(m - 1, 0), m, m + 1):
        texts.append("".join(rng.choice(list(letters + "xy"), n)))                   # x, y: outside the alphabet
    texts += [pattern, pattern[:m // 2] + "x" + pattern[m // 2:], pattern[1:], "x" * 70]
    lay = tmx.text_layout(texts, [pattern], raw=True)
    peq = R.peq_tables(lay.pattern_ids.tolist(), lay.alphabet)
    assert len(peq) == (m + 63) // 64
    for i, text in enumerate(texts):
        a, b = lay.span(i, 1)
        assert lay.text[a:b] == text
        assert R.myers_distance(peq, m, lay.page_ids[a:b].tolist()) == R.dp_distance(text, pattern), (m, len(text))


def test_enumeration_edges():
    assert R.candidates(5, 1) == [(1, i, 1) for i in range(5)] + [(2, i, 2) for i in range(4)]        # g = 1: size 0 dropped
    assert R.candidates(3, 3) == [(0, 0, 2), (0, 1, 2), (1, 0, 3)]                                      # g + 1 > N
    assert R.candidates(1, 1) == [(1, 0, 1)] and R.candidates(1, 2) == [(0, 0, 1)] and R.candidates(1, 3) == []   # N = 1
    lines = [1, 1, 2, 2, 2]
    assert R.candidates(5, 2, []) == R.candidates(5, 2, None)                                          # [] is falsy: no rule
    assert R.candidates(5, 2, lines) == [(0, i, 1) for i in range(5)] + [(1, 0, 2), (1, 2, 2), (1, 3, 2), (2, 2, 3)]


# ---------------------------------------------------------------------------------------------------- predict on the host
def _vector(key: bytes) -> np.ndarray:
    return np.random.default_rng(list(key[:64]) + [len(key)]).standard_normal(16)


def _embed_text(text):
    return _vector(text.encode("utf-8"))


def _embed_clip(clip):
    return _vector(bytes(clip[::16, ::16].tobytes()))


def _clip_of(snippet):
    """a host stand-in for the device resize: the snippet tiled over 224 x 224"""
    reps = (224 // snippet.shape[0] + 1, 224 // snippet.shape[1] + 1, 1)
    return np.ascontiguousarray(np.tile(snippet, reps)[:224, :224])


class HostMatcher(tmx.MetaTemplateMatcher):
    """MetaTemplateMatcher with the two device calls supplied on the host: the kernel's tables by the DP, the resize by tiling"""

    def __init__(self):
        tmx.BaseTemplateMatcher.__init__(self, False)
        self.embeddings_processor, self.text_embeddings_processor = _embed_clip, _embed_text
        self.embedding_cache, self.cached_embeddings_clips, self.ctx = {}, {}, None

    def _clip(self, snippet):
        return _clip_of(snippet)


@pytest.fixture()
def host_kernel(monkeypatch):
    def tables(ctx, layout, g, line_ids=None):
        off, N = layout.pattern_off, len(layout.ws)
        patterns = [layout.pattern_ids[off[t]:off[t + 1]].tolist() for t in range(len(off) - 1)]
        dist = np.full((len(patterns), 3, N), -1, np.int32)
        length = np.full((len(patterns), 3, N), -1, np.int32)
        for t, p in enumerate(patterns):
            for k, i, n in R.candidates(N, int(g[t]), line_ids):
                a, b = layout.span(i, n)
                dist[t, k, i], length[t, k, i] = R.dp_distance(layout.page_ids[a:b].tolist(), p), b - a
        return dist, length

    monkeypatch.setattr(tmx, "lev_ngrams_host", tables)


def _page():
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (96, 256, 3)).astype(np.uint8)
    words = ["invoice", "total", "due", "Invoice", "totel", "amount", "paid", "total"]
    boxes = [[8 + 30 * (k % 4), 10 + 40 * (k // 4), 26, 12] for k in range(len(words))]
    lines = [1 + k // 4 for k in range(len(words))]
    tframe = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
    return frame, words, boxes, lines, tframe


def _both(host, frame, tframes, tboxes, labels, texts, thr, words, boxes, lines):
    got = host.predict(frame, tframes, tboxes, labels, texts, thr, words=words, word_boxes=boxes, word_lines=lines)
    totals = []
    want = R.predict(R.Scorer(_embed_text, _embed_clip, _clip_of), frame, tframes, tboxes, labels, texts, thr, words, boxes, lines,
                     totals)
    assert [(list(p.bbox), p.label, p.score) for p in got] == [(list(b), l, s) for b, l, s in want]
    assert all(p.similarity == p.score for p in got)
    return got, totals


def test_predict_equals_the_restatement(host_kernel):
    frame, words, boxes, lines, tframe = _page()
    host = HostMatcher()
    texts = ["Invoice total", " total ", "absent words", "ab", None]
    labels = ["head", "sum", "none", "short", "null"]
    for thr in (0.9, 0.6, 0.3, 0.05):
        for ln in (lines, [], None):
            got, totals = _both(host, frame, [tframe] * 5, [(4, 4, 40, 20)] * 5, labels, texts, thr, words, boxes, ln)
            print(thr, ln is not None and len(ln), [(p.label, p.bbox, p.score) for p in got], len(totals))
            assert {p.label for p in got} <= {"head", "sum", "none"}          # "ab" and None are skipped
    assert host.predict(frame, [tframe], [(4, 4, 40, 20)], ["a"], ["total"], 0.9, words=None, word_boxes=boxes) == []
    assert host.predict(frame, [tframe], [(4, 4, 40, 20)], ["a"], ["total"], 0.9, words=words, word_boxes=None) == []
    assert host.predict(frame, [tframe], [(4, 4, 40, 20)], ["a"], ["total"], 0.9, words=[], word_boxes=[]) == []
    with pytest.raises(AssertionError):
        host.predict(frame, [tframe], [(4, 4, 40, 20)], ["a"], ["total"], 0.9, words=words, word_boxes=boxes[:-1])
    with pytest.raises(ValueError, match="template_texts"):
        host.predict(frame, [tframe], [(4, 4, 40, 20)], ["a"], None, 0.9, words=words, word_boxes=boxes)


def test_equal_strings_are_accepted_below_the_threshold(host_kernel):
    frame, words, boxes, lines, tframe = _page()
    host = HostMatcher()
    got, totals = _both(host, frame, [tframe], [(4, 4, 40, 20)], ["sum"], ["DUE"], 1.0, words, boxes, lines)
    assert [p.bbox for p in got] == [boxes[2]] and got[0].score < 1.0         # nothing exceeds 1.0; "due" equals the text
    assert max(totals) < 1.0


def test_suppression_is_per_label_and_order_is_by_ngram_size(host_kernel):
    frame, words, boxes, lines, tframe = _page()
    host = HostMatcher()
    args = ([tframe] * 2, [(4, 4, 40, 20)] * 2)
    # at a threshold of -1 every candidate passes: the smallest n-gram size comes first and shuts out what overlaps it
    one, _ = _both(host, frame, *args, ["x", "x"], ["invoice total", "total due"], -1.0, words, boxes, lines)
    two, _ = _both(host, frame, *args, ["x", "y"], ["invoice total", "total due"], -1.0, words, boxes, lines)
    assert [p.bbox for p in one[:len(words)]] == boxes                         # g - 1 = 1: the single words, in page order
    assert all(p.label == "x" for p in one) and len(one) == len(words)         # every longer n-gram overlaps one of them
    assert [p.label for p in two] == ["x"] * len(words) + ["y"] * len(words)   # the other label is not shut out by them
    assert tmx.is_overlap((0, 0, 10, 10), (9, 9, 5, 5)) and not tmx.is_overlap((0, 0, 10, 10), (10, 0, 5, 5))


# ---------------------------------------------------------------------------------------------------- run
class StubMatcher(tmx.BaseTemplateMatcher):
    def __init__(self):
        super().__init__(False)
        self.calls = []

    def predict(self, frame, template_frames, template_boxes, template_labels, template_texts=None, score_threshold=0.9,
                scoring_strategy="weighted", max_objects=1, batch_size=1, words=None, word_boxes=None, word_lines=None):
        self.calls.append((frame.shape, words, word_boxes, word_lines))
        if not words:
            return []
        return [tmx.TemplateMatchResult(bbox=word_boxes[0], label=template_labels[0], score=0.95, similarity=0.95)]


def test_run_hands_the_words_of_each_page_to_predict():
    frames = [np.zeros((40, 60, 3), np.uint8), np.zeros((50, 70, 3), np.uint8)]
    metadata = [{"words": [{"text": "a", "box": [1, 2, 3, 4], "line": 1}, {"text": "b", "box": [5, 6, 7, 8], "line": 2}]},
                {"words": [{"text": "c", "box": [9, 9, 9, 9], "line": 1}]}]
    tframe = np.zeros((16, 24, 3), np.uint8)
    stub = StubMatcher()
    out = stub.run(frames, [tframe], [(0, 0, 8, 8)], ["t"], ["text"], metadata=metadata, window_size=(16, 24))
    assert stub.calls == [((40, 60, 3), ["a", "b"], [[1, 2, 3, 4], [5, 6, 7, 8]], [1, 2]), ((50, 70, 3), ["c"], [[9, 9, 9, 9]], [1])]
    assert [(r.bbox, r.frame_index) for r in out] == [([1, 2, 3, 4], 0), ([9, 9, 9, 9], 1)]
    for none in (None, []):
        stub.calls.clear()
        assert stub.run(frames[:1], [tframe], [(0, 0, 8, 8)], ["t"], ["text"], metadata=none, window_size=(16, 24)) == []
        assert stub.calls == [((40, 60, 3), None, None, None)]
    # through the composite, which hands metadata on
    stub.calls.clear()
    out = tmx.CompositeTemplateMatcher([stub]).run(frames, [tframe], [(0, 0, 8, 8)], ["t"], ["text"], metadata=metadata,
                                                   window_size=(16, 24))
    assert [c[1] for c in stub.calls] == [["a", "b"], ["c"]] and sorted(r.frame_index for r in out) == [0, 1]


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    with pytest.raises(ValueError, match="embeddings_processor"):
        tmx.MetaTemplateMatcher("meta", ctx=object())
    with pytest.raises(ValueError, match="text"):
        tmx.MetaTemplateMatcher("meta", embeddings_processor=_embed_clip, ctx=object())
    with pytest.raises(MarieHipError, match="use_gpu"):
        tmx.MetaTemplateMatcher("meta", use_gpu=False, embeddings_processor=_embed_clip, text_embeddings_processor=_embed_text)
    m = tmx.MetaTemplateMatcher("meta", embeddings_processor=_embed_clip, text_embeddings_processor=_embed_text, ctx=object())
    assert m.slicing_enabled is False and m.embedding_cache == {} and m.cached_embeddings_clips == {}
    frame, words, boxes, lines, tframe = _page()
    with pytest.raises(ValueError, match="1025 code points"):                 # before any launch: the context is a dummy
        m.predict(frame, [tframe], [(4, 4, 40, 20)], ["long"], ["A" * 1025], 0.9, words=words, word_boxes=boxes)
    with pytest.raises(ValueError, match="bit table"):
        distinct = "".join(chr(0x4E00 + k) for k in range(1024))             # 1,024 distinct letters x 16 words: 128 KiB
        m.predict(frame, [tframe], [(4, 4, 40, 20)], ["wide"], [distinct], 0.9, words=words, word_boxes=boxes)
