"""Seeded cases of the document indexer's post-model procedure (test infrastructure): pages of words with a label per word, cut
into windows by the product tokeniser, and per-window logits that say those labels with a chosen confidence.  The golden
generator (tools/gen_indexer_golden.py) runs the reference's own code on them; tests/test_indexer_cpu.py runs the product's and
the restatement's and compares with what the generator stored in tests/golden/indexer.json."""
from __future__ import annotations

import os
import tempfile

import numpy as np

WIDTH, HEIGHT = 1700, 2200
_ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


def marie_config():
    from marie_icr_amd.weights import make_indexer_config

    return make_indexer_config(0, 2)


_TOK = None


def tokenizer():
    global _TOK
    if _TOK is None:
        from marie_icr_amd.document_classifier import ByteLevelBPE
        from marie_icr_amd.weights import write_synthetic_bpe

        d = tempfile.mkdtemp(prefix="indexer_bpe_")
        write_synthetic_bpe(d, seed=1)
        _TOK = ByteLevelBPE(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"))
    return _TOK


def _layout(rng, lines):
    """lines: [[(n_words, key or None), ...]] left to right -> words, boxes (x, y, w, h) in pixels, keys per word.  A segment
    given as (n_words, key, x) starts at pixel x instead of after the previous one."""
    words, boxes, keys = [], [], []
    y = 40
    for line in lines:
        x = 30
        for seg in line:
            n, key = seg[0], seg[1]
            if len(seg) > 2:
                x = seg[2]
            for _ in range(n):
                w = "".join(_ALPHABET[int(i)] for i in rng.integers(0, len(_ALPHABET), int(rng.integers(2, 9))))
                bw = 11 * len(w)
                words.append(w)
                boxes.append([x, y + int(rng.integers(0, 3)), bw, 24])
                keys.append(key)
                x += bw + 14
        y += 40
    return words, boxes, keys


def _case(name, seed, lines, n_windows, disturb=None, duplicate=()):
    """``disturb(window, word index, key, label index)`` -> (label index, confidence) lets a case make windows disagree."""
    from marie_icr_amd.document_indexer import normalize_bbox

    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    labels = marie_config()["labels"]
    words, boxes, keys = _layout(rng, lines)
    for a, b in duplicate:                       # word b takes the box of word a
        boxes[b] = list(boxes[a])
    norm = [normalize_bbox(b, (WIDTH, HEIGHT)) for b in boxes]
    tok = tokenizer()
    ids, bbox, mask, first = tok.encode_windows(words, norm)
    assert ids.shape[0] == n_windows, (name, ids.shape[0])
    # word of every sub-token, in page order
    word_of = [k for k, w in enumerate(words) for _ in tok.encode_word(w)]
    word_label = []
    prev = None
    for k, key in enumerate(keys):
        word_label.append(0 if key is None else labels.index(("I-" if prev == key else "B-") + key))
        prev = key
    windows = []
    for w in range(ids.shape[0]):
        n_sub = int(mask[w].sum()) - 2
        start = w * (510 - 128)
        lab = np.zeros((512,), np.int64)
        conf = np.zeros((512,), np.float32)
        for i in range(n_sub):
            k = word_of[start + i]
            li, c = word_label[k], 6.0 + float((k * 7 + w * 3) % 5)
            if disturb is not None:
                li, c = disturb(w, k, keys[k], li, c)
            lab[1 + i], conf[1 + i] = li, c
        windows.append({"labels": lab, "conf": conf, "bbox": bbox[w], "first": first[w], "seed": 100 * seed + w})
    return {"name": name, "width": WIDTH, "height": HEIGHT, "words": words, "boxes": boxes, "boxes_norm": norm, "keys": keys,
            "windows": windows}


def case_arrays(case):
    """-> {"logits" [n][512][L] fp32 (multiples of 1/8 plus the confidence on the label), "bbox" [n][512][4], "first" [n][512]}"""
    L = len(marie_config()["labels"])
    logits = []
    for w in case["windows"]:
        rng = np.random.Generator(np.random.PCG64(w["seed"]))
        z = rng.integers(-8, 9, size=(512, L)).astype(np.float32) / 8
        z[np.arange(512), w["labels"]] += w["conf"]
        logits.append(z)
    return {"logits": np.stack(logits), "bbox": np.stack([w["bbox"] for w in case["windows"]]),
            "first": np.stack([w["first"] for w in case["windows"]])}


def make_cases():
    cfg = marie_config()
    (q0, a0), (q1, a1) = [(p[0], p[1][0]) for p in cfg["expected_pair"]]
    filler = [[(9, None)] for _ in range(3)]
    form = [[(2, q0), (3, a0), (2, None), (1, q1), (2, a1)], [(4, None)], [(3, "NAME")], [(4, "ADDRESS")], [(2, "ADDRESS")]]
    cases = [_case("one_window", 1, form + filler, 1)]

    long_page = [[(2, q0), (3, a0), (4, None)]] + [[(10, None)] for _ in range(6)] + [[(1, q1), (2, a1), (6, None)]] + \
                [[(10, q0 if r % 5 == 0 else None)] for r in range(13)]

    def conflict(w, k, key, li, c):
        # a later window sees every third word differently: sometimes surer, sometimes less sure, sometimes exactly as sure
        if w > 0 and k % 3 == 0:
            return (li + 1) % 13, c + (1.0, -1.0, 0.0)[(k // 3) % 3]
        return li, c

    cases.append(_case("three_windows_conflict", 2, long_page, 3, disturb=conflict))
    cases.append(_case("duplicate_boxes", 3, form + filler, 1, duplicate=((0, 1), (5, 6), (12, 13))))
    left = [[(2, a0, 30), (2, q0, 700)], [(2, q1, 30), (2, a1, 500)], [(5, None)]]
    cases.append(_case("answer_left_of_question", 4, left, 1))
    entity = [[(3, "NAME", 100)], [(4, "ADDRESS", 100)], [(3, "ADDRESS", 100)], [(6, None)], [(6, None)], [(6, None)], [(6, None)],
              [(2, "NAME", 900)], [(3, "ADDRESS", 900)]]
    cases.append(_case("composite_entity", 5, entity, 1))
    return cases
