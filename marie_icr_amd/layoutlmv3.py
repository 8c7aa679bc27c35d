"""LayoutLMv3 model (page classifier and token tagger): binding of the ``mhip_layoutlmv3_*`` entry points (include/marie_hip.h).

reference: ``LayoutLMv3ForSequenceClassification`` of the transformers library as ``TransformersDocumentClassifier`` drives it
(marie/components/document_classifier/transformers.py:159-172, :300-361).  The tokeniser and the classifier surface are in
``document_classifier.py``; this file is the model handle: pages + token ids + boxes + mask in, logits (and, for tests, the
last hidden states and the resized pages) out.  For the document indexer (``LayoutLMv3ForTokenClassification`` as
marie/components/document_indexer/transformers.py:519-568 drives it; surface in ``document_indexer.py``) the same handle tags
windows of text: ``tag_device`` / ``tag_host`` return one label and one score per token.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from ._lib import PREC_F16, AttentionHostDesc, Context, CropDesc, LayoutLMv3Config, ModelHandle, check, load

# the Pillow filters of the page resize (MHIP_PIL_* of include/marie_hip.h = PIL.Image.LANCZOS / BILINEAR / BICUBIC)
PIL_LANCZOS, PIL_BILINEAR, PIL_BICUBIC = 1, 2, 3

# config.json keys that map one to one onto mhip_layoutlmv3_config fields
_CONFIG_KEYS = {"hidden_size": "hidden", "num_hidden_layers": "layers", "num_attention_heads": "heads",
                "intermediate_size": "ffn", "vocab_size": "vocab", "type_vocab_size": "type_vocab",
                "max_position_embeddings": "max_position_embeddings",
                "max_2d_position_embeddings": "max_2d_position_embeddings", "coordinate_size": "coordinate_size",
                "shape_size": "shape_size", "input_size": "input_size", "patch_size": "patch", "rel_pos_bins": "rel_pos_bins",
                "max_rel_pos": "max_rel_pos", "rel_2d_pos_bins": "rel_2d_pos_bins", "max_rel_2d_pos": "max_rel_2d_pos",
                "layer_norm_eps": "layer_norm_eps", "pad_token_id": "pad_id"}


def default_config(lib=None, **overrides) -> LayoutLMv3Config:
    """The base checkpoint's configuration (``mhip_layoutlmv3_default_config``), fields overridden by keyword."""
    cfg = LayoutLMv3Config()
    rc = (lib or load()).mhip_layoutlmv3_default_config(C.byref(cfg))
    if rc:
        raise ValueError(f"mhip_layoutlmv3_default_config -> {rc}")
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise ValueError(f"unknown LayoutLMv3 config field {k}")
        setattr(cfg, k, v)
    return cfg


def config_from_hf(hf: dict, lib=None) -> LayoutLMv3Config:
    """``config.json`` of a LayoutLMv3 checkpoint -> ``LayoutLMv3Config``.  What the kernels do not cover is refused here or at
    create: no text-only / image-only variants, no attention without both relative biases."""
    for flag in ("visual_embed", "text_embed", "has_relative_attention_bias", "has_spatial_attention_bias"):
        if not hf.get(flag, True):
            raise ValueError(f"LayoutLMv3 config with {flag}=false is not supported")
    if hf.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"LayoutLMv3 hidden_act {hf.get('hidden_act')!r} is not supported")
    if hf.get("num_channels", 3) != 3:
        raise ValueError("LayoutLMv3 num_channels must be 3")
    cfg = default_config(lib)
    for k, f in _CONFIG_KEYS.items():
        if k in hf:
            setattr(cfg, f, hf[k])
    if "id2label" in hf:
        cfg.num_labels = len(hf["id2label"])
    elif "num_labels" in hf:
        cfg.num_labels = int(hf["num_labels"])
    return cfg


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)


def pack_pages(pages: Sequence[np.ndarray]):
    """Pages (H x W x 3 uint8, any sizes) -> one packed buffer and its ``CropDesc`` array."""
    descs = (CropDesc * len(pages))()
    total = 0
    for i, p in enumerate(pages):
        if p.ndim != 3 or p.shape[2] != 3 or p.dtype != np.uint8:
            raise ValueError(f"page {i}: expected an H x W x 3 uint8 array, got {p.shape} {p.dtype}")
        h, w = p.shape[:2]
        descs[i] = CropDesc(total, h, w, w * 3, 3)
        total += (h * w * 3 + 255) // 256 * 256
    packed = np.zeros((total,), np.uint8)
    for i, p in enumerate(pages):
        packed[descs[i].src_offset: descs[i].src_offset + p.size] = np.ascontiguousarray(p).reshape(-1)
    return packed, descs


class LayoutLMv3Model(ModelHandle):
    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], config: LayoutLMv3Config,
                 precision: int = PREC_F16):
        self.cfg, self.precision = config, int(precision)
        super().__init__(ctx, "layoutlmv3", self.precision, C.byref(config))
        self.seq_len = self.lib.mhip_layoutlmv3_seq_len(C.byref(config))
        if state is not None:
            self.load_state(state)

    def set_resample(self, filter: int) -> None:
        """The Pillow filter of the page resize for every later call: ``PIL_LANCZOS`` (the document splitter's image
        processor), ``PIL_BILINEAR`` (the default) or ``PIL_BICUBIC``; anything else raises."""
        self._call("set_resample", int(filter))

    def _inputs(self, n, ids, bbox, mask):
        T = self.cfg.max_text
        ids = np.ascontiguousarray(ids, np.int32).reshape(n, T)
        bbox = np.ascontiguousarray(bbox, np.int32).reshape(n, T, 4)
        mask = np.ascontiguousarray(mask, np.int32).reshape(n, T)
        return ids, bbox, mask

    def classify_device(self, base_ptr: int, descs, n: int, ids, bbox, mask) -> np.ndarray:
        """n pages inside one device buffer -> logits (n, num_labels), one model call."""
        ids, bbox, mask = self._inputs(n, ids, bbox, mask)
        logits = np.empty((n, self.cfg.num_labels), np.float32)
        check(self.ctx.h, self.lib.mhip_layoutlmv3_classify(self.h, C.c_void_p(base_ptr), descs, n, _vp(ids), _vp(bbox),
                                                            _vp(mask), _vp(logits)), "mhip_layoutlmv3_classify")
        return logits

    def forward_host(self, pages: Sequence[np.ndarray], ids, bbox, mask, want_hidden: bool = False,
                     want_resized: bool = False) -> dict:
        """Host pages -> {"logits"} (+ "hidden" (n, seq_len, hidden) fp32: the last hidden states, every row;
        + "resized" (n, input_size, input_size, 3) uint8)."""
        n = len(pages)
        packed, descs = pack_pages(pages)
        ids, bbox, mask = self._inputs(n, ids, bbox, mask)
        S = self.cfg.input_size
        logits = np.empty((n, self.cfg.num_labels), np.float32)
        hidden = np.empty((n, self.seq_len, self.cfg.hidden), np.float32) if want_hidden else None
        resized = np.empty((n, S, S, 3), np.uint8) if want_resized else None
        check(self.ctx.h, self.lib.mhip_layoutlmv3_hidden_host(self.h, _vp(packed), packed.size, descs, n, _vp(ids), _vp(bbox),
                                                               _vp(mask), _vp(logits), _vp(hidden), _vp(resized)),
              "mhip_layoutlmv3_hidden_host")
        out = {"logits": logits}
        if want_hidden:
            out["hidden"] = hidden
        if want_resized:
            out["resized"] = resized
        return out


    def _windows(self, n_pages: int, window_page, ids, bbox, mask):
        wp = np.ascontiguousarray(window_page, np.int32).reshape(-1)
        n = int(wp.size)
        if n < 1 or wp.min() < 0 or wp.max() >= n_pages:
            raise ValueError(f"window_page must name pages 0..{n_pages - 1} for at least one window")
        return (wp, n) + self._inputs(n, ids, bbox, mask)

    def _tag_out(self, n: int, want_logits: bool):
        T = self.cfg.max_text
        labels, scores = np.empty((n, T), np.int32), np.empty((n, T), np.float32)
        logits = np.empty((n, T, self.cfg.num_labels), np.float32) if want_logits else None
        return labels, scores, logits

    def tag_device(self, base_ptr: int, descs, n_pages: int, window_page, ids, bbox, mask, want_logits: bool = False) -> dict:
        """Windows of text over ``n_pages`` pages inside one device buffer (window w belongs to page ``window_page[w]``)
        -> {"labels" (n_win, max_text) int32, "scores" (n_win, max_text) fp32} (+ "logits" (n_win, max_text, num_labels)),
        one model call; the pages are resized and projected once each."""
        wp, n, ids, bbox, mask = self._windows(n_pages, window_page, ids, bbox, mask)
        labels, scores, logits = self._tag_out(n, want_logits)
        check(self.ctx.h, self.lib.mhip_layoutlmv3_tag(self.h, C.c_void_p(base_ptr), descs, n_pages, _vp(wp), n, _vp(ids), _vp(bbox),
                                                       _vp(mask), _vp(labels), _vp(scores), _vp(logits)), "mhip_layoutlmv3_tag")
        out = {"labels": labels, "scores": scores}
        if want_logits:
            out["logits"] = logits
        return out

    def tag_host(self, pages: Sequence[np.ndarray], window_page, ids, bbox, mask, want_logits: bool = False) -> dict:
        """``tag_device`` on host pages."""
        packed, descs = pack_pages(pages)
        wp, n, ids, bbox, mask = self._windows(len(pages), window_page, ids, bbox, mask)
        labels, scores, logits = self._tag_out(n, want_logits)
        check(self.ctx.h, self.lib.mhip_layoutlmv3_tag_host(self.h, _vp(packed), packed.size, descs, len(pages), _vp(wp), n, _vp(ids),
                                                            _vp(bbox), _vp(mask), _vp(labels), _vp(scores), _vp(logits)),
              "mhip_layoutlmv3_tag_host")
        out = {"labels": labels, "scores": scores}
        if want_logits:
            out["logits"] = logits
        return out


def token_head_host(ctx: Context, precision: int, hidden, out_w, out_b, dense_w=None, dense_b=None, want_logits: bool = True):
    """The token head alone (``mhip_token_head_host``): hidden (rows, D) fp32, ``out_w`` (L, D), ``out_b`` (L) and, for the
    dense head, ``dense_w`` (D, D) + ``dense_b`` (D) -> (labels int32 (rows), scores fp32 (rows), logits fp32 (rows, L) or None)."""
    hidden = np.ascontiguousarray(hidden, np.float32)
    rows, D = hidden.shape
    out_w, out_b = np.ascontiguousarray(out_w, np.float32), np.ascontiguousarray(out_b, np.float32)
    L = out_w.shape[0]
    if dense_w is not None:
        dense_w, dense_b = np.ascontiguousarray(dense_w, np.float32), np.ascontiguousarray(dense_b, np.float32)
    labels, scores = np.empty((rows,), np.int32), np.empty((rows,), np.float32)
    logits = np.empty((rows, L), np.float32) if want_logits else None
    check(ctx.h, ctx.lib.mhip_token_head_host(ctx.h, int(precision), rows, D, L, _vp(hidden), _vp(dense_w), _vp(dense_b), _vp(out_w),
                                              _vp(out_b), _vp(labels), _vp(scores), _vp(logits)), "mhip_token_head_host")
    return labels, scores, logits


def attention_bias_host(ctx: Context, precision: int, q, k, v, pos, x, y, valid, w1, wx, wy, max_1d: int = 128,
                        max_2d: int = 256) -> np.ndarray:
    """The biased attention kernel alone (``mhip_attention_bias_host``): q / k / v (n_tok, heads * 64) fp32, per-token
    position / x / y / valid, the three head-major bias matrices -> (n_tok, heads * 64) fp32."""
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    n_tok, D = q.shape
    pos, x, y, valid = (np.ascontiguousarray(a, np.int32) for a in (pos, x, y, valid))
    w1, wx, wy = (np.ascontiguousarray(a, np.float32) for a in (w1, wx, wy))
    out = np.empty((n_tok, D), np.float32)
    check(ctx.h, ctx.lib.mhip_attention_bias_host(ctx.h, int(precision), D // 64, n_tok, _vp(q), _vp(k), _vp(v), _vp(pos),
                                                  _vp(x), _vp(y), _vp(valid), _vp(w1), _vp(wx), _vp(wy), w1.shape[1],
                                                  int(max_1d), wx.shape[1], int(max_2d), _vp(out)),
          "mhip_attention_bias_host")
    return out


ATTN_SLACK_ROWS = 128          # MHIP_ATTN_SLACK_ROWS
ATTN_LAYOUT_FUSED, ATTN_LAYOUT_SPLIT = 0, 1


def attention_host(ctx: Context, precision: int, layout: int, images: int, heads: int, n_queries: int, n_keys: int, npad_q: int,
                   npad_k: int, q, k, vt, bias: Optional[dict] = None) -> np.ndarray:
    """One launch of the plain or biased attention kernel with the whole descriptor in the caller's hands
    (``mhip_attention_host``).  q (images * npad_q + 128, heads * 64), k (images * npad_k + 128, heads * 64) and vt
    (heads * 64 * images * npad_k + 128,) fp32, every padding and slack row the caller's; ``bias``: qcode (rows, 3) and kcode
    (rows, 4) int32, w1 / wx / wy, max_1d, max_2d, dp, dx.  -> the device's whole output (images * npad_q + 128, heads * 64) in
    the element type (float16 / float32), pre-filled with the byte 0xff."""
    q, k, vt = (np.ascontiguousarray(a, np.float32) for a in (q, k, vt))
    D = max(int(heads), 0) * 64
    rq, rk = max(int(images) * int(npad_q), 0) + ATTN_SLACK_ROWS, max(int(images) * int(npad_k), 0) + ATTN_SLACK_ROWS
    if q.size != rq * D or k.size != rk * D or vt.size != D * (rk - ATTN_SLACK_ROWS) + ATTN_SLACK_ROWS:
        raise ValueError("attention_host: q / k / vt do not have the rows the descriptor names")
    out = np.zeros((rq, D), np.float16 if int(precision) == PREC_F16 else np.float32)
    d = AttentionHostDesc(precision=int(precision), layout=int(layout), images=int(images), heads=int(heads), n_queries=int(n_queries),
                          n_keys=int(n_keys), npad_q=int(npad_q), npad_k=int(npad_k), q=_vp(q), k=_vp(k), vt=_vp(vt), out=_vp(out))
    keep = []
    if bias is not None:
        qc, kc = np.ascontiguousarray(bias["qcode"], np.int32), np.ascontiguousarray(bias["kcode"], np.int32)
        w1, wx, wy = (np.ascontiguousarray(bias[n], np.float32) for n in ("w1", "wx", "wy"))
        if qc.shape != (rq, 3) or kc.shape != (rk, 4) or w1.shape[0] != heads or wx.shape != wy.shape or wx.shape[0] != heads:
            raise ValueError("attention_host: bias operands do not have the rows the descriptor names")
        keep = [qc, kc, w1, wx, wy]
        d.qcode, d.kcode, d.w1, d.wx, d.wy = (_vp(a) for a in keep)
        d.bins_1d, d.bins_2d = w1.shape[1], wx.shape[1]
        d.max_1d, d.max_2d, d.dp, d.dx = (int(bias[n]) for n in ("max_1d", "max_2d", "dp", "dx"))
    check(ctx.h, ctx.lib.mhip_attention_host(ctx.h, C.byref(d)), "mhip_attention_host")
    return out
