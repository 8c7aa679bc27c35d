"""LayoutReader reading order: ``TextLayout`` of the reference (marie/document/layoutreader/text_layout.py), whose model is
``LayoutlmForSeq2SeqDecoder`` (marie/models/unilm/layoutreader/s2s_ft/modeling_decoding.py) run greedily
(``search_beam_size == 1``, ``pos_shift=False``) in layout-only mode: the words are never embedded, only their boxes are.

    layout = TextLayout("/models/layoutreader")            # config.json + pytorch_model.bin / model.safetensors
    words, boxes = layout(words, boxes)                    # boxes: x0, y0, x1, y1 in 0 .. 1000 (the LayoutLM normalisation)

``forward`` returns the model's raw index list (``argmax - 1`` per step: -1 is [CLS], ``len(words)`` is [SEP], larger values
are pad rows), ``reconstruct`` turns it into an order as the reference does, and ``forward_batch`` runs several pages through
one model call.  There is no CPU path (``use_gpu=False`` raises) and no tokenizer: a layout-only model needs no vocabulary.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import PREC_F16, PREC_F32, Context, LayoutReaderConfig, MarieHipError, ModelHandle, check

logger = logging.getLogger(__name__)

BOX_MAX = 1000
MAX_PAGES = 64          # pages of one model call

_DROPPED = ("bert.pooler.", "cls.seq_relationship.")
_UNBUILT = (("num_qkv", lambda v: int(v or 0) > 1), ("seg_emb", bool), ("ffn_type", lambda v: int(v or 0) != 0),
            ("relax_projection", lambda v: int(v or 0) > 1), ("new_pos_ids", bool))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().float().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=np.float32)


def layoutreader_keys(cfg: LayoutReaderConfig) -> Dict[str, Tuple[int, ...]]:
    """every tensor the model of ``cfg`` takes (checkpoint names) -> its shape"""
    D, F = cfg.dim, cfg.ffn
    keys: Dict[str, Tuple[int, ...]] = {"bert.embeddings.position_embeddings.weight": (cfg.max_position, D)}
    for name in "xyhw":
        keys[f"bert.embeddings.{name}_position_embeddings.weight"] = (cfg.max_2d, D)
    keys["bert.embeddings.token_type_embeddings.weight"] = (cfg.type_vocab, D)
    keys["bert.embeddings.LayerNorm.weight"] = keys["bert.embeddings.LayerNorm.bias"] = (D,)
    for n in range(cfg.depth):
        p = f"bert.encoder.layer.{n}."
        for name, o, i in (("attention.self.query", D, D), ("attention.self.key", D, D), ("attention.self.value", D, D),
                           ("attention.output.dense", D, D), ("intermediate.dense", F, D), ("output.dense", D, F)):
            keys[p + name + ".weight"] = (o, i)
            if name != "attention.self.key":        # F.linear(x, key.weight): the model never reads key.bias
                keys[p + name + ".bias"] = (o,)
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            keys[p + name + ".weight"] = keys[p + name + ".bias"] = (D,)
    keys["cls.predictions.bias"] = (cfg.max_source,)
    keys["cls.predictions.transform.dense.weight"] = (D, D)
    keys["cls.predictions.transform.dense.bias"] = (D,)
    keys["cls.predictions.transform.LayerNorm.weight"] = keys["cls.predictions.transform.LayerNorm.bias"] = (D,)
    return keys


def config_from_json(config: Dict[str, Any]) -> LayoutReaderConfig:
    """``config.json`` of a LayoutReader checkpoint -> the geometry.  Options of the s2s-ft code base the layout-only greedy
    decoder does not use raise ``NotImplementedError``, named."""
    for name, on in _UNBUILT:
        if on(config.get(name)):
            raise NotImplementedError(f"LayoutReader config.json: {name}={config.get(name)!r} is not built")
    base = str(config.get("base_model_type", "layoutlm"))
    if base != "layoutlm":
        raise NotImplementedError(f"LayoutReader config.json: base_model_type {base!r} (layoutlm is built)")
    act = str(config.get("hidden_act", "gelu"))
    if act != "gelu":
        raise NotImplementedError(f"LayoutReader config.json: hidden_act {act!r} (the erf GELU is built)")
    cfg = LayoutReaderConfig()
    try:
        cfg.dim, cfg.heads = int(config["hidden_size"]), int(config["num_attention_heads"])
        cfg.depth, cfg.ffn = int(config["num_hidden_layers"]), int(config["intermediate_size"])
    except KeyError as e:
        raise MarieHipError(f"LayoutReader config.json: no {e.args[0]}") from None
    cfg.max_position = int(config.get("max_position_embeddings", 1024))
    cfg.max_2d = int(config.get("max_2d_position_embeddings", 1024))
    cfg.max_source = int(config.get("max_source_length", 513))
    cfg.type_vocab = int(config.get("type_vocab_size", 2))
    cfg.source_type, cfg.target_type = int(config.get("source_type_id", 0)), int(config.get("target_type_id", 1))
    cfg.ln_eps = 1e-5          # BertLayerNorm(eps=1e-5) wherever the model builds one; layer_norm_eps is not read
    return cfg


def load_layoutreader_state(state_dict: Dict[str, Any], config: Dict[str, Any]) -> Tuple[Dict[str, np.ndarray], LayoutReaderConfig]:
    """A loaded LayoutReader checkpoint and its ``config.json`` -> (the model's tensors as float32 arrays, the geometry).
    ``gamma`` / ``beta`` become ``weight`` / ``bias`` as ``from_pretrained`` renames them; ``bert.pooler.*``,
    ``cls.seq_relationship.*``, every ``key.bias`` and any ``word_embeddings`` are dropped (the layout-only greedy decoder reads
    none of them).  A missing or misshapen tensor raises :class:`MarieHipError`, named."""
    sd = state_dict.get("model_state_dict", state_dict) if isinstance(state_dict, dict) else None
    if not isinstance(sd, dict) or not sd:
        raise MarieHipError("LayoutReader checkpoint: expected a state dict or {'model_state_dict': state dict}")
    cfg = config_from_json(config)
    named = {}
    for key, val in sd.items():
        key = key.replace("gamma", "weight").replace("beta", "bias")
        if key.startswith("module."):
            key = key[7:]
        if not key.startswith(("bert.", "cls.")):
            key = "bert." + key
        if key.startswith(_DROPPED) or key.endswith("attention.self.key.bias") or "word_embeddings" in key:
            continue
        named[key] = val
    state = {}
    for key, shape in layoutreader_keys(cfg).items():
        if key not in named:
            raise MarieHipError(f"LayoutReader checkpoint: no {key}")
        arr = _f32(named[key])
        if arr.shape != shape:
            raise MarieHipError(f"LayoutReader checkpoint: {key} has shape {arr.shape}, the configuration asks for {shape}")
        state[key] = arr
    return state, cfg


class LayoutReaderModel(ModelHandle):
    """``mhip_layoutreader``: the encoder, the pointer decoder and its caches on a :class:`Context`."""

    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], config: LayoutReaderConfig, precision: int = PREC_F16):
        self.cfg, self.precision = config, int(precision)
        super().__init__(ctx, "layoutreader", self.precision, C.byref(config))
        if state is not None:
            self.load_state(state)

    @property
    def steps(self) -> int:
        return self.cfg.max_source - 2

    def _pages(self, pages) -> Tuple[np.ndarray, np.ndarray]:
        S = self.cfg.max_source
        if not 1 <= len(pages) <= MAX_PAGES:
            raise ValueError(f"1 .. {MAX_PAGES} pages a call, got {len(pages)}")
        boxes = np.zeros((len(pages), S - 2, 4), np.int32)
        counts = np.zeros(len(pages), np.int32)
        for i, b in enumerate(pages):
            b = check_boxes(b, S - 2)
            boxes[i, :len(b)] = b
            counts[i] = len(b)
        return boxes, counts

    def workspace_bytes(self, pages: int) -> int:
        return int(self.lib.mhip_layoutreader_workspace_bytes(self.h, int(pages)))

    def order_host(self, pages) -> np.ndarray:
        """pages: a list of int boxes (n, 4) -> decisions int32 (pages, T), indices into the S source rows"""
        boxes, counts = self._pages(pages)
        out = np.empty((len(counts), self.steps), np.int32)
        self._call("order_host", _vp(boxes), _vp(counts), len(counts), _vp(out))
        return out

    def debug_host(self, pages, forced=None) -> Dict[str, np.ndarray]:
        """-> dict(decisions (pages, T), scores (pages, T, S), emb (pages, S, dim) the embedded source rows, last (pages, S, dim)
        the last layer's output of the source pass, zeros past [SEP]).  forced int (pages, T): step t + 1 is fed source row
        forced[page][t]; the decisions and scores reported are still the kernels' own"""
        boxes, counts = self._pages(pages)
        P, T, S, D = len(counts), self.steps, self.cfg.max_source, self.cfg.dim
        if forced is not None:
            forced = np.ascontiguousarray(forced, np.int32)
            if forced.shape != (P, T):
                raise ValueError(f"forced indices of shape {(P, T)} expected, got {forced.shape}")
        out = dict(decisions=np.empty((P, T), np.int32), scores=np.empty((P, T, S), np.float32), emb=np.empty((P, S, D), np.float32),
                   last=np.empty((P, S, D), np.float32))
        self._call("debug_host", _vp(boxes), _vp(counts), P, _vp(forced), _vp(out["decisions"]), _vp(out["scores"]), _vp(out["emb"]),
                   _vp(out["last"]))
        return out


def decode_attention_host(ctx: Context, precision: int, q, k, v, kc, vc, src_len, tgt_len, heads: int, tgt_base: int) -> np.ndarray:
    """The decode attention kernel alone.  q, k, v fp32 (pages, nq, heads * 64): the rows a step feeds, q already scaled by
    1/8 * log2(e); kc, vc fp32 (pages, cache_rows, heads * 64); src_len int (pages,), tgt_len int (pages, nq).  Query row i sees
    cache rows < src_len, cache rows tgt_base + [0, tgt_len) and rows 0 .. i of k / v -> fp32 (pages, nq, heads * 64)"""
    q, k, v, kc, vc = (np.ascontiguousarray(a, np.float32) for a in (q, k, v, kc, vc))
    P, nq, D = q.shape
    src_len = np.ascontiguousarray(src_len, np.int32).reshape(-1)
    tgt_len = np.ascontiguousarray(tgt_len, np.int32).reshape(-1)
    if (D != heads * 64 or k.shape != q.shape or v.shape != q.shape or kc.ndim != 3 or kc.shape[0] != P or kc.shape[2] != D or
            vc.shape != kc.shape or src_len.shape[0] != P or tgt_len.shape[0] != P * nq):
        raise ValueError(f"q, k, v (pages, nq, heads * 64), caches (pages, rows, heads * 64), lengths (pages,) and (pages, nq) "
                         f"expected, got {q.shape}, {k.shape}, {v.shape}, {kc.shape}, {vc.shape}, {src_len.shape}, {tgt_len.shape}")
    out = np.empty_like(q)
    check(ctx.h, ctx.lib.mhip_layoutreader_attention_host(ctx.h, int(precision), _vp(q), _vp(k), _vp(v), _vp(kc), _vp(vc), _vp(src_len),
                                                          _vp(tgt_len), P, nq, int(heads), kc.shape[1], int(tgt_base), _vp(out)),
          "mhip_layoutreader_attention_host")
    return out


def check_boxes(boxes, max_words: int) -> np.ndarray:
    """boxes of one page -> int32 (n, 4); ``ValueError`` for more than ``max_words``, a coordinate outside 0 .. 1000 or an
    inverted box (the model would index its tables with them)"""
    b = np.asarray(boxes)
    if b.size == 0:
        return np.zeros((0, 4), np.int32)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"boxes of shape (n, 4) expected, got {b.shape}")
    if len(b) > max_words:
        raise ValueError(f"{len(b)} words: the model takes {max_words} a page")
    if not np.issubdtype(b.dtype, np.integer):
        if not np.all(b == np.floor(b)):
            raise ValueError("boxes must be whole numbers (x0, y0, x1, y1 normalised to 0 .. 1000)")
    b = b.astype(np.int64)
    if b.min() < 0 or b.max() > BOX_MAX:
        raise ValueError(f"box coordinates must lie in 0 .. {BOX_MAX}, got {int(b.min())} .. {int(b.max())}")
    if np.any(b[:, 2] < b[:, 0]) or np.any(b[:, 3] < b[:, 1]):
        raise ValueError("a box has x1 < x0 or y1 < y0")
    return b.astype(np.int32)


def reorder(words: Sequence, boxes: Sequence, idx: Sequence[int]):
    """``TextLayout.reconstruct`` behind the model call, as it stands (text_layout.py:208-226): duplicates dropped in first-seen
    order; when that does not leave one index a word, indices >= len(words) are dropped, the unused ones are appended in
    ascending order and the count is asserted; then numpy fancy indexing — in which a -1 ([CLS]) names the last word."""
    processed_idx = list(dict.fromkeys(int(i) for i in idx))
    if len(processed_idx) != len(words):
        processed_idx = [i for i in processed_idx if i < len(words)]
        unused_idx = sorted(list(set(range(len(words))) - set(processed_idx[: len(words)])))
        logger.info(f"There is {len(words)} words but only {len(processed_idx)} indexes. Unmatched indexes: {unused_idx}")
        processed_idx.extend(unused_idx)
        assert len(processed_idx) == len(words)
    out_words = list(np.array(words)[processed_idx])
    out_boxes = [elem.tolist() for elem in np.array(boxes)[processed_idx]]
    return out_words, out_boxes


class TextLayout:
    """marie/document/layoutreader/text_layout.py:31-231.  ``model_path`` is a local directory with ``config.json`` and the
    weights; ``state`` (a state dict) + ``config`` (the config.json dict) stand in for it."""

    def __init__(self, model_path: Optional[str] = None, *, state: Optional[Dict[str, Any]] = None, config: Optional[Dict[str, Any]] = None,
                 precision: str = "f16", ctx: Optional[Context] = None, use_gpu: bool = True):
        if not use_gpu:
            raise MarieHipError("TextLayout runs on the GPU only: there is no CPU path in this project")
        if precision not in ("f16", "f32"):
            raise ValueError(f"precision {precision!r}: 'f16' or 'f32'")
        if state is None:
            if model_path is None:
                raise ValueError("TextLayout needs a model directory, or state= and config=")
            from .document_classifier import _load_state

            with open(os.path.join(model_path, "config.json"), "r", encoding="utf-8") as f:
                config = dict(json.load(f), **(config or {}))
            state = _load_state(model_path)
        elif config is None:
            raise ValueError("state= needs config= (the config.json dict)")
        tensors, cfg = load_layoutreader_state(state, config)
        self.ctx = ctx if ctx is not None else Context(0)
        self.model = LayoutReaderModel(self.ctx, tensors, cfg, PREC_F16 if precision == "f16" else PREC_F32)
        self.max_len = cfg.max_source - 2          # 511 in production: max_tgt_length
        self.beam_size = 1

    def close(self):
        self.model.close()

    def __call__(self, *args, **kwargs):
        return self.reconstruct(*args, **kwargs)

    def forward_batch(self, pages: Sequence) -> List[List[int]]:
        """several pages' boxes through one model call (the decoder's GEMMs then have 2 x pages rows over one read of the
        weights) -> the index list of every page, as ``forward`` returns it"""
        out: List[List[int]] = []
        pages = list(pages)
        for at in range(0, len(pages), MAX_PAGES):
            dec = self.model.order_host(pages[at:at + MAX_PAGES])
            out.extend((row - 1).tolist() for row in dec.astype(np.int64))
        return out

    def forward(self, words: Sequence[str], boxes: Sequence[Sequence[int]]) -> List[int]:
        """the model's index list for one page: ``argmax - 1`` of every one of the T steps"""
        assert len(words) == len(boxes)
        return self.forward_batch([boxes])[0]

    def reconstruct(self, words: List[str], boxes: List[List[int]]) -> Tuple[List[str], List[List[int]]]:
        assert len(words) == len(boxes)
        if len(words) > self.max_len:
            logging.warning(f"Page contains {len(words)} words. Exceeds the {self.max_len} limit and will not be reordered.")
            return words, boxes
        return reorder(words, boxes, self.forward(words, boxes))
