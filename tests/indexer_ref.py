"""Restatement of the document indexer's model call and of its post-model procedure (test infrastructure: the GPU tests compare
the HIP tagger against it, the CPU tests compare it against the transformers library in float64 and against the golden file the
reference's own code wrote).

Follows transformers/models/layoutlmv3/modeling_layoutlmv3.py (LayoutLMv3ForTokenClassification.forward: the head on
``sequence_output[:, :seq_length]``; ``nn.Linear`` for ``num_labels < 10``, else LayoutLMv3ClassificationHead with
``pool_feature=False``) and marie/components/document_indexer/transformers.py:556-666.
"""
from __future__ import annotations

import numpy as np
import torch

import layoutlmv3_ref as R


def head_kind(state) -> str:
    return "linear" if "classifier.weight" in state else "dense"


def token_logits(state, hidden_text: torch.Tensor, round_f16: bool = False) -> torch.Tensor:
    """The token head on text rows [..., D] in their dtype.  ``round_f16``: the dense matrix rounded to f16, as the f16 model
    holds it (tanh, out_proj and everything after are fp32 there in both modes)."""
    dt = hidden_text.dtype
    lin = torch.nn.functional.linear

    def W(k, r=False):
        t = torch.as_tensor(np.asarray(state[k])).to(dt)
        return t.to(torch.float16).to(dt) if r else t

    if head_kind(state) == "linear":
        return lin(hidden_text, W("classifier.weight"), W("classifier.bias"))
    y = torch.tanh(lin(hidden_text, W("classifier.dense.weight", round_f16), W("classifier.dense.bias")))
    return lin(y, W("classifier.out_proj.weight"), W("classifier.out_proj.bias"))


def forward(state, cfg: dict, input_ids, bbox, attention_mask, pixel_values, dtype=torch.float64, round_f16: bool = False):
    """LayoutLMv3ForTokenClassification.forward -> (last hidden states [n][T + G*G + 1][D], logits [n][T][labels]).
    ``pixel_values`` [n][3][S][S]: one image per window, as the library takes them."""
    st = state
    if head_kind(state) == "linear":      # the encoder restatement also evaluates the row-0 head: give it one to evaluate
        D = cfg["hidden_size"]
        st = dict(state)
        st["classifier.dense.weight"], st["classifier.dense.bias"] = np.zeros((D, D), np.float32), np.zeros((D,), np.float32)
        st["classifier.out_proj.weight"], st["classifier.out_proj.bias"] = np.zeros((1, D), np.float32), np.zeros((1,), np.float32)
    hidden, _ = R.forward(st, cfg, input_ids, bbox, attention_mask, pixel_values, dtype, round_f16)
    T = np.asarray(input_ids).shape[1]
    return hidden, token_logits(state, hidden[:, :T], round_f16)


def decide(logits: np.ndarray):
    """(arg-max, soft-max probability of the arg-max) as ``logits.argmax(-1)`` / ``logits.softmax(-1)`` give them, evaluated in
    the logits' own precision"""
    t = torch.as_tensor(logits)
    pred = t.argmax(-1)
    prob = torch.softmax(t, dim=-1).gather(-1, pred.unsqueeze(-1)).squeeze(-1)
    return pred.numpy(), prob.numpy()


def post_model(labels, words, boxes_norm, width, height, logits, win_bbox, win_first):
    """transformers.py:559-666 from the logits of a page's windows on -> (predictions, boxes, scores) per word.  Written apart
    from the product's ``merge_window_predictions`` (lists of records here) so that the two check each other against the golden."""
    pred, prob = decide(np.asarray(logits, np.float32))
    merged = []          # [label, box, score] in the order tokens were first seen
    for w in range(len(pred)):
        keep = [i for i in range(len(pred[w])) if win_first[w][i]]
        lab = [labels[int(pred[w][i])] for i in keep]
        box = [[int(width * (win_bbox[w][i][0] / 1000)), int(height * (win_bbox[w][i][1] / 1000)),
                int(width * (win_bbox[w][i][2] / 1000)), int(height * (win_bbox[w][i][3] / 1000))] for i in keep]
        sc = [round(float(prob[w][i]), 6) for i in keep]
        nz = [k for k, b in enumerate(box) if b != [0, 0, 0, 0]]
        lab, box = [lab[k] for k in nz], [box[k] for k in nz]
        sc = sc[:len(box)]                      # the reference filters the scores against the filtered boxes: a prefix survives
        it = 0
        while it < len(box):                    # "for box in true_boxes" with pops inside
            b = box[it]
            if box.count(b) > 1:
                at = box.index(b)
                del lab[at], box[at], sc[at]
            it += 1
        if w > 0:
            for rec in merged:
                if rec[1] in box:
                    at = box.index(rec[1])
                    if sc[at] >= rec[2]:
                        rec[0], rec[2] = lab[at], sc[at]
                    del lab[at], box[at], sc[at]
        merged.extend([a, b, c] for a, b, c in zip(lab, box, sc))
    seen = [m[1] for m in merged]
    out = ([], [], [])
    for bn in boxes_norm:
        ob = [int(v) for v in (width * (bn[0] / 1000), height * (bn[1] / 1000), width * (bn[2] / 1000), height * (bn[3] / 1000))]
        if ob not in seen:
            raise ValueError(f"Box not found for alignment: {ob}")
        m = merged[seen.index(ob)]
        out[0].append(m[0]); out[1].append(m[1]); out[2].append(m[2])
    return out


# ------------------------------------------------------------------------------------------------ shared test pages
def make_words(seed: int, n_subtokens: int, tokenizer, width: int, height: int, exact: bool = False):
    """Seeded OCR-like words on a grid of lines (boxes x, y, w, h in pixels, all different) whose sub-token count reaches
    ``n_subtokens`` (``exact``: is exactly that, by shortening the last word)."""
    rng = np.random.Generator(np.random.PCG64(seed + 613))
    alphabet = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    words, boxes, total = [], [], 0
    per_line = 12
    while total < n_subtokens:
        k = len(words)
        w = "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(1, 10))))
        n = len(tokenizer.encode_word(w))
        if exact:
            while total + n > n_subtokens:
                w = w[:-1]
                n = len(tokenizer.encode_word(w))
        col, row = k % per_line, k // per_line
        cw, lh = width // per_line, max(height // 64, 6)
        words.append(w)
        boxes.append([col * cw + int(rng.integers(0, 3)), 8 + row * (lh + 4), cw - 6 - int(rng.integers(0, 3)), lh])
        total += n
    return words, boxes


INDEX_PAGE_SUBTOKENS = (300, 520, 1000)         # 1, 2 (the second mostly padding) and 3 windows


def make_index_pages(tokenizer, sizes=((1100, 850), (1320, 1020), (1100, 850))):
    """Three seeded pages with 1 + 2 + 3 windows: [(page uint8 HxWx3, words, boxes xywh in pixels)]."""
    from marie_icr_amd.weights import make_page_bgr

    out = []
    for i, (n_sub, (h, w)) in enumerate(zip(INDEX_PAGE_SUBTOKENS, sizes)):
        words, boxes = make_words(50 + i, n_sub, tokenizer, w, h)
        out.append((make_page_bgr(700 + i, h, w), words, boxes))
    return out


def encode_index_pages(pages, tokenizer):
    """-> window_page [n_win], ids, bbox, mask, first (all windows of all pages), and the normalised boxes per page"""
    from marie_icr_amd.document_indexer import normalize_bbox

    wp, parts, norm = [], [], []
    for k, (page, words, boxes) in enumerate(pages):
        nb = [normalize_bbox(b, (page.shape[1], page.shape[0])) for b in boxes]
        e = tokenizer.encode_windows(words, nb)
        wp += [k] * e[0].shape[0]
        parts.append(e)
        norm.append(nb)
    cat = [np.concatenate([p[j] for p in parts]) for j in range(4)]
    return np.asarray(wp, np.int32), cat[0], cat[1], cat[2], cat[3], norm
