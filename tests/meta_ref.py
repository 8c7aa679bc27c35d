"""MetaTemplateMatcher in plain Python, one pair at a time as the reference runs it
(marie/components/template_matching/meta_template_matching.py): the textbook edit distance, the page-as-one-string layout, the
n-gram enumeration, ``score`` and ``predict``.  The embedders and the 224 x 224 framing come in as callables."""
import numpy as np


def dp_distance(a, b) -> int:
    """Wagner-Fischer with two rows, unit costs, over the items of two sequences (code points of two str)"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[len(b)]


def dp_distance_rows(a, b) -> int:
    """``dp_distance`` with each row in numpy, for the long strings of the GPU tests (equal to it: tests/test_meta_cpu.py).
    cur[j] = min(prev[j] + 1, prev[j - 1] + cost, cur[j - 1] + 1): the last term is a running minimum of cur[j] - j"""
    a = np.frombuffer(a.encode("utf-32-le", "surrogatepass"), np.uint32) if isinstance(a, str) else np.asarray(a)
    b = np.frombuffer(b.encode("utf-32-le", "surrogatepass"), np.uint32) if isinstance(b, str) else np.asarray(b)
    ramp = np.arange(len(b) + 1)
    prev = ramp.copy()
    for i, x in enumerate(a, 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(cur - ramp) + ramp
    return int(prev[len(b)])


# ---------------------------------------------------------------------------------------------------- layout
def layout(words, patterns):
    """S, per-word (ws, we, fs, le), the alphabet (sorted code points of the patterns) and the ids of S, one character at a
    time"""
    S = " ".join(w.upper() for w in words)
    ws, we, at = [], [], 0
    for w in words:
        ws.append(at)
        we.append(at + len(w.upper()))
        at = we[-1] + 1
    fs, le = [], []
    for a, b in zip(ws, we):
        p = a
        while p < len(S) and S[p].isspace():
            p += 1
        fs.append(p)
        q = b
        while q > 0 and S[q - 1].isspace():
            q -= 1
        le.append(q)
    letters = sorted(set("".join(patterns)))
    ident = {ch: k + 1 for k, ch in enumerate(letters)}
    return dict(S=S, ws=ws, we=we, fs=fs, le=le, letters=letters, page_ids=[ident.get(ch, 0) for ch in S],
                pattern_ids=[[ident[ch] for ch in p] for p in patterns])


def span(lay, i, n):
    a = min(lay["fs"][i], lay["we"][i + n - 1])
    return a, max(lay["le"][i + n - 1], a)


def ngram_text(words, i, n) -> str:
    return " ".join(words[i:i + n]).strip().upper()


def candidates(n_words, g, word_lines=None):
    """(k, i, n) of every n-gram the reference scores for a template of ``g`` words (:152-176)"""
    out = []
    for k, n in enumerate((g - 1, g, g + 1)):
        if not 0 < n <= n_words:
            continue
        for i in range(n_words - n + 1):
            if word_lines and len(set(word_lines[i:i + n])) > 1:
                continue
            out.append((k, i, n))
    return out


def expected_tables(words, patterns, gs, word_lines=None, distance=dp_distance, memo=None):
    """dist, len int32 (T, 3, N) as the kernel reports them, by the DP on the reference's strings; ``memo`` keeps the distances
    of (text, pattern) pairs across calls"""
    N = len(words)
    dist = np.full((len(patterns), 3, N), -1, np.int32)
    length = np.full((len(patterns), 3, N), -1, np.int32)
    memo = {} if memo is None else memo
    for t, (p, g) in enumerate(zip(patterns, gs)):
        for k, i, n in candidates(N, g, word_lines):
            text = ngram_text(words, i, n)
            if (text, p) not in memo:
                memo[text, p] = distance(text, p)
            dist[t, k, i], length[t, k, i] = memo[text, p], len(text)
    return dist, length


# ---------------------------------------------------------------------------------------------------- Myers, blocked
MASK = (1 << 64) - 1


def peq_tables(pattern_ids, alphabet):
    """Peq[w][id]: bit j % 64 of word j // 64 set where pattern[j] == id; id 0 matches nothing"""
    W = (len(pattern_ids) + 63) // 64
    peq = [[0] * (alphabet + 1) for _ in range(W)]
    for j, c in enumerate(pattern_ids):
        assert 1 <= c <= alphabet
        peq[j // 64][c] |= 1 << (j % 64)
    return peq


def myers_distance(peq, m, text_ids) -> int:
    """Myers' bit-vector algorithm in Hyyro's blocked form over 64-bit words, as csrc/lev_ngrams.hip runs it"""
    if m == 0:
        return len(text_ids)
    W = len(peq)
    Pv, Mv, score = [MASK] * W, [0] * W, m
    wl, top = (m - 1) // 64, 1 << ((m - 1) % 64)
    for c in text_ids:
        hin = 1
        for w in range(W):
            Eq = peq[w][c]
            Xv = Eq | Mv[w]
            if hin < 0:
                Eq |= 1
            Xh = ((((Eq & Pv[w]) + Pv[w]) & MASK) ^ Pv[w]) | Eq
            Ph = (Mv[w] | ~(Xh | Pv[w])) & MASK
            Mh = Pv[w] & Xh
            if w == wl:
                score += 1 if Ph & top else (-1 if Mh & top else 0)
            hout = 1 if Ph >> 63 else (-1 if Mh >> 63 else 0)
            Ph = ((Ph << 1) | (1 if hin > 0 else 0)) & MASK
            Mh = ((Mh << 1) | (1 if hin < 0 else 0)) & MASK
            Pv[w] = (Mh | ~(Xv | Ph)) & MASK
            Mv[w] = Ph & Xv
            hin = hout
    return score


# ---------------------------------------------------------------------------------------------------- score and predict
def merge_bboxes_as_block(bboxes):
    """marie/utils/overlap.py:186-204"""
    b = np.array(bboxes)
    min_x, min_y = b[:, 0].min(), b[:, 1].min()
    return [round(k, 6) for k in [min_x, min_y, (b[:, 0] + b[:, 2]).max() - min_x, (b[:, 1] + b[:, 3]).max() - min_y]]


def cosine(a, b) -> float:
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.dot(a, b) / (max(np.linalg.norm(a), 1e-8) * max(np.linalg.norm(b), 1e-8)))


class Scorer:
    """``score`` (:270-311) with the reference's two caches; ``embed_text`` text -> vector, ``embed_clip`` 224 x 224 clip ->
    vector, ``clip_of`` snippet -> 224 x 224 clip (resize_image)"""

    def __init__(self, embed_text, embed_clip, clip_of):
        self.embed_text, self.embed_clip, self.clip_of = embed_text, embed_clip, clip_of
        self.embedding_cache, self.cached_embeddings_clips = {}, {}

    def get_embedding(self, text):
        if text not in self.embedding_cache:
            self.embedding_cache[text] = self.embed_text(text[:1024])
        return self.embedding_cache[text]

    def get_embedding_image(self, clip):
        key = clip.tobytes()
        if key not in self.cached_embeddings_clips:
            assert clip.shape[:2] == (224, 224)
            self.cached_embeddings_clips[key] = self.embed_clip(clip)
        return self.cached_embeddings_clips[key]

    def terms(self, ngram_words, template_text, query_snippet, template_snippet):
        """(lev, cos_text, cos_image, total); the cosines None below lev 0.5"""
        d = dp_distance(ngram_words, template_text)
        lev = 1 - d / max(len(ngram_words), len(template_text))
        if lev < 0.5:
            return lev, None, None, lev
        cos_image = cosine(self.get_embedding_image(self.clip_of(template_snippet)),
                           self.get_embedding_image(self.clip_of(query_snippet)))
        cos_text = cosine(self.get_embedding(ngram_words), self.get_embedding(template_text))
        return lev, cos_text, cos_image, (lev + cos_text + cos_image) / 3

    def score(self, ngram_words, template_text, query_snippet, template_snippet) -> float:
        return self.terms(ngram_words, template_text, query_snippet, template_snippet)[3]


def predict(scorer, frame, template_frames, template_boxes, template_labels, template_texts, score_threshold, words, word_boxes,
            word_lines=None, totals=None):
    """:98-237 -> [(bbox, label, score)]; ``totals`` (a list) receives every unrounded score"""
    predictions = []
    if words is None or word_boxes is None:
        return predictions
    assert len(words) == len(word_boxes) and len(template_frames) == len(template_boxes)
    assert len(template_texts) == len(template_labels)
    for idx, (template_text, template_label) in enumerate(zip(template_texts, template_labels)):
        if template_text is None or len(template_text) < 3:
            continue
        tx, ty, tw, th = template_boxes[idx]
        tx, ty = int(max(tx, 0)), int(max(ty, 0))
        fragment = template_frames[idx][ty:ty + th, tx:tx + tw]
        g = len(template_text.split(" "))
        found = []
        for _, i, n in candidates(len(words), g, word_lines):
            box = merge_bboxes_as_block(word_boxes[i:i + n])
            x, y, w, h = box
            ngram_words = ngram_text(words, i, n)
            template_text = template_text.strip().upper()
            total = scorer.score(ngram_words, template_text, frame[y:y + h, x:x + w], fragment)
            if totals is not None:
                totals.append(total)
            sim_val = round(total, 3)
            if ngram_words == template_text or sim_val > score_threshold:
                found.append((n, (box, template_label, sim_val)))
        for _, cand in sorted(found, key=lambda e: e[0]):
            x1, y1, w1, h1 = cand[0]
            for bbox, label, _ in predictions:
                x2, y2, w2, h2 = bbox
                if cand[1] == label and (x1 < x2 + w2 and x1 + w1 > x2 and y1 < y2 + h2 and y1 + h1 > y2):
                    break
            else:
                predictions.append(cand)
    return predictions
