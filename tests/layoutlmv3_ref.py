"""Plain-torch restatement of LayoutLMv3ForSequenceClassification's forward and of the tokeniser / box-expansion rules of the
page classifier, parameterised by dtype (test infrastructure: the GPU tests compare the HIP model against it, the CPU tests
compare it against the transformers library in float64).

Follows transformers/models/layoutlmv3/modeling_layoutlmv3.py: LayoutLMv3TextEmbeddings, LayoutLMv3Model.forward_image /
forward, LayoutLMv3Encoder (relative_position_bucket, _cal_1d_pos_emb, _cal_2d_pos_emb), LayoutLMv3SelfAttention (the "cogview"
soft-max is the plain soft-max), LayoutLMv3Layer, LayoutLMv3ClassificationHead.
"""
from __future__ import annotations

import math

import numpy as np
import torch

BASE_CFG = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=50265,
                type_vocab_size=1, max_position_embeddings=514, max_2d_position_embeddings=1024, coordinate_size=128,
                shape_size=128, input_size=224, patch_size=16, rel_pos_bins=32, max_rel_pos=128, rel_2d_pos_bins=64,
                max_rel_2d_pos=256, layer_norm_eps=1e-5, pad_token_id=1, num_labels=7)


def relative_position_bucket(relative_position: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """LayoutLMv3Encoder.relative_position_bucket(bidirectional=True), its float32 arithmetic included."""
    num_buckets //= 2
    ret = (relative_position > 0).long() * num_buckets
    n = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    val_if_large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact)
                                * (num_buckets - max_exact)).to(torch.long)
    val_if_large = torch.min(val_if_large, torch.full_like(val_if_large, num_buckets - 1))
    return ret + torch.where(is_small, n, val_if_large)


def visual_bbox(grid: int, max_len: int = 1000) -> torch.Tensor:
    """LayoutLMv3Model.create_visual_bbox: the cls box, then the grid x grid patch boxes on 0..max_len."""
    edges = torch.div(torch.arange(0, max_len * (grid + 1), max_len), grid, rounding_mode="trunc")
    rows = []
    for py in range(grid):
        for px in range(grid):
            rows.append([int(edges[px]), int(edges[py]), int(edges[px + 1]), int(edges[py + 1])])
    return torch.tensor([[1, 1, max_len - 1, max_len - 1]] + rows, dtype=torch.long)


def pixel_values_from_pages(pages, size: int = 224):
    """LayoutLMv3ImageProcessor(apply_ocr=False, do_resize=True, resample=BILINEAR) on frames as the reference passes them
    (channel order as stored): PIL BILINEAR resize, x / 255, (x - 0.5) / 0.5 -> (float64 [n][3][size][size], resized uint8)."""
    from PIL import Image

    resized = np.stack([np.asarray(Image.fromarray(p).resize((size, size), Image.BILINEAR)) for p in pages])
    x = (resized.astype(np.float64) / 255.0 - 0.5) / 0.5
    return torch.from_numpy(x).permute(0, 3, 1, 2).contiguous(), resized


def _r16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(t.dtype)


def forward(state, cfg: dict, input_ids, bbox, attention_mask, pixel_values, dtype=torch.float64, round_f16: bool = False):
    """-> (last hidden states [n][T + G*G + 1][D], logits [n][labels]).  ``round_f16``: the f16 stand-in — matrix weights and
    every layer's output rounded to f16, arithmetic in ``dtype``."""
    D, H = cfg["hidden_size"], cfg["num_attention_heads"]
    eps, pad = cfg["layer_norm_eps"], cfg["pad_token_id"]
    G = cfg["input_size"] // cfg["patch_size"]
    rnd = _r16 if round_f16 else (lambda t: t)

    def W(k, matrix=False):
        t = torch.as_tensor(np.asarray(state[k])).to(dtype)
        return rnd(t) if matrix else t

    def ln(x, prefix, e):
        return torch.nn.functional.layer_norm(x, (D,), W(prefix + ".weight"), W(prefix + ".bias"), e)

    ids = torch.as_tensor(np.asarray(input_ids)).long()
    bb = torch.as_tensor(np.asarray(bbox)).long()
    am = torch.as_tensor(np.asarray(attention_mask)).long()
    n, T = ids.shape
    E = "layoutlmv3.embeddings."
    nonpad = (ids != pad).long()
    pos_ids = torch.cumsum(nonpad, dim=1) * nonpad + pad
    emb = rnd(W(E + "word_embeddings.weight"))[ids] + W(E + "token_type_embeddings.weight")[0]
    emb = emb + W(E + "position_embeddings.weight")[pos_ids]
    xe, ye = W(E + "x_position_embeddings.weight"), W(E + "y_position_embeddings.weight")
    he, we = W(E + "h_position_embeddings.weight"), W(E + "w_position_embeddings.weight")
    spatial = torch.cat([xe[bb[..., 0]], ye[bb[..., 1]], xe[bb[..., 2]], ye[bb[..., 3]],
                         he[torch.clip(bb[..., 3] - bb[..., 1], 0, 1023)], we[torch.clip(bb[..., 2] - bb[..., 0], 0, 1023)]], dim=-1)
    text = ln(emb + spatial, E + "LayerNorm", eps)
    pv = pixel_values.to(dtype)
    patches = torch.nn.functional.conv2d(rnd(pv), W("layoutlmv3.patch_embed.proj.weight", True), W("layoutlmv3.patch_embed.proj.bias"),
                                         stride=cfg["patch_size"]).flatten(2).transpose(1, 2)
    vis = torch.cat([W("layoutlmv3.cls_token").expand(n, -1, -1), patches], dim=1) + W("layoutlmv3.pos_embed")
    vis = ln(vis, "layoutlmv3.norm", 1e-6)
    x = rnd(ln(torch.cat([text, vis], dim=1), "layoutlmv3.LayerNorm", eps))
    NV = G * G + 1
    pos = torch.cat([torch.arange(T), torch.arange(NV)]).unsqueeze(0).expand(n, -1)
    fb = torch.cat([bb, visual_bbox(G).unsqueeze(0).expand(n, -1, -1)], dim=1)
    keep = torch.cat([am, torch.ones((n, NV), dtype=torch.long)], dim=1).bool()
    rel = relative_position_bucket(pos.unsqueeze(-2) - pos.unsqueeze(-1), cfg["rel_pos_bins"], cfg["max_rel_pos"])
    rx = relative_position_bucket(fb[:, :, 0].unsqueeze(-2) - fb[:, :, 0].unsqueeze(-1), cfg["rel_2d_pos_bins"], cfg["max_rel_2d_pos"])
    ry = relative_position_bucket(fb[:, :, 3].unsqueeze(-2) - fb[:, :, 3].unsqueeze(-1), cfg["rel_2d_pos_bins"], cfg["max_rel_2d_pos"])
    e = "layoutlmv3.encoder."
    bias = (W(e + "rel_pos_bias.weight").t()[rel] + (W(e + "rel_pos_x_bias.weight").t()[rx] + W(e + "rel_pos_y_bias.weight").t()[ry]))
    bias = bias.permute(0, 3, 1, 2) / 8.0
    bias = bias.masked_fill(~keep[:, None, None, :], float("-inf"))
    lin = torch.nn.functional.linear
    for i in range(cfg["num_hidden_layers"]):
        p = f"layoutlmv3.encoder.layer.{i}."

        def heads(t):
            return t.view(n, -1, H, 64).transpose(1, 2)

        q = heads(lin(x, W(p + "attention.self.query.weight", True), W(p + "attention.self.query.bias")))
        k = heads(lin(x, W(p + "attention.self.key.weight", True), W(p + "attention.self.key.bias")))
        v = heads(lin(x, W(p + "attention.self.value.weight", True), W(p + "attention.self.value.bias")))
        probs = torch.softmax(torch.matmul(q / 8.0, k.transpose(-1, -2)) + bias, dim=-1)
        ctx = rnd(torch.matmul(probs, v).permute(0, 2, 1, 3).reshape(n, -1, D))
        x = rnd(ln(lin(ctx, W(p + "attention.output.dense.weight", True), W(p + "attention.output.dense.bias")) + x,
                   p + "attention.output.LayerNorm", eps))
        hid = rnd(torch.nn.functional.gelu(lin(x, W(p + "intermediate.dense.weight", True), W(p + "intermediate.dense.bias"))))
        x = rnd(ln(lin(hid, W(p + "output.dense.weight", True), W(p + "output.dense.bias")) + x, p + "output.LayerNorm", eps))
    y = torch.tanh(lin(x[:, 0], W("classifier.dense.weight"), W("classifier.dense.bias")))
    logits = lin(y, W("classifier.out_proj.weight"), W("classifier.out_proj.bias"))
    return x, logits


# ------------------------------------------------------------------------------------------------ tokeniser rules
def encode_page_rules(words, boxes, encode_word, bos: int, eos: int, pad: int, max_length: int = 512):
    """The box-expansion / special-box / truncation / padding rules of LayoutLMv3Tokenizer(words, boxes=...,
    max_length, padding="max_length", truncation=True), restated over any word encoder."""
    ids, bbs = [], []
    for w, b in zip(words, boxes):
        sub = list(encode_word(w))
        ids += sub
        bbs += [list(b)] * len(sub)
    ids, bbs = ids[: max_length - 2], bbs[: max_length - 2]
    ids = [bos] + ids + [eos]
    bbs = [[0, 0, 0, 0]] + bbs + [[0, 0, 0, 0]]
    mask = [1] * len(ids) + [0] * (max_length - len(ids))
    bbs += [[0, 0, 0, 0]] * (max_length - len(ids))
    ids += [pad] * (max_length - len(ids))
    return np.asarray(ids, np.int32), np.asarray(bbs, np.int32).reshape(max_length, 4), np.asarray(mask, np.int32)


def scale_boxes(boxes, width: int, height: int):
    ws, hs = 1000 / width, 1000 / height
    return [[int(b[0] * ws), int(b[1] * hs), int(b[2] * ws), int(b[3] * hs)] for b in boxes]


# ------------------------------------------------------------------------------------------------ shared test pages
TEST_PAGE_LINES = (0, 3, 12, 25, 40, 60, 80, 10)      # OCR lines per page: no text at all ... far more than 512 sub-tokens


def make_test_pages(n: int = 8, small_last: bool = True):
    """Seeded pages with OCR words and boxes: 2550 x 3300 frames (the last one small), text lengths from none to > 512
    sub-tokens.  -> [(page uint8 HxWx3, words, boxes)]"""
    from marie_icr_amd.renderer import get_words_and_boxes
    from marie_icr_amd.weights import make_ocr_result, make_page_bgr

    out = []
    for i in range(n):
        h, w = (330, 255) if (small_last and i == n - 1) else (3300, 2550)
        page = make_page_bgr(100 + i, h, w)
        lines = TEST_PAGE_LINES[i % len(TEST_PAGE_LINES)]
        if lines:
            words, boxes = get_words_and_boxes([make_ocr_result(200 + i, w, h, n_lines=lines)], 0)
        else:
            words, boxes = [], []
        out.append((page, words, boxes))
    return out


def encode_test_pages(pages, tokenizer):
    """ids / bbox / mask arrays of ``make_test_pages`` output through the product tokeniser and the reference's box scaling."""
    ids, bbox, mask = [], [], []
    for page, words, boxes in pages:
        i, b, m = tokenizer.encode_page(words, scale_boxes(boxes, page.shape[1], page.shape[0]))
        ids.append(i); bbox.append(b); mask.append(m)
    return np.stack(ids), np.stack(bbox), np.stack(mask)
