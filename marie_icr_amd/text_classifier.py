"""The text-only page classifier: Longformer sequence classification over the OCR words of a page.

reference: ``TransformersDocumentClassifier`` with ``task="text-classification"`` (marie/components/document_classifier/
transformers.py:223-258; the task ``setup_classifiers`` of marie/pipe/components.py defaults to), which hands ``" ".join(words)`` of
every page to ``pipeline("text-classification", top_k=..., truncation=True)``; and, for what the reference delegates to the
transformers library, ``LongformerTokenizer`` (RoBERTa's byte-level BPE), ``LongformerForSequenceClassification`` with global
attention on ``<s>`` alone, and the pipeline's post-processing (soft-max, or sigmoid for one label / multi-label models).

The model runs in HIP on the ``mhip_berttext`` handle (csrc/berttext_api.hip: ``attn_window``, ``attn_global_row``,
``cls_head``); only logits and scores come back.  Pages are sorted into length buckets, a bucket is one model call; a page's
logits do not depend on its bucket, bit for bit.  A model directory holds ``config.json`` (``model_type: "longformer"``),
``model.safetensors`` or ``pytorch_model.bin``, ``vocab.json`` + ``merges.txt`` and, optionally, ``tokenizer_config.json``
(``model_max_length``).
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import PREC_F16, PREC_F32, Context, MarieHipError, ModelHandle, SentenceEncoderConfig, TextClassifierConfig, check
from .document_classifier import ByteLevelBPE, _load_state
from .embeddings import BertTextModel, plan_text_groups

HEAD_NONE, HEAD_SOFTMAX, HEAD_SIGMOID = 0, 1, 2
MAX_WINDOW = 512          # one-sided, attn_window's


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def head_function_of(config: Dict[str, Any], num_labels: int) -> int:
    """the pipeline's choice (TextClassificationPipeline.postprocess): sigmoid for one label or a multi-label model, soft-max
    otherwise; a regression head has no scores and is refused by name"""
    problem = config.get("problem_type")
    if problem == "regression":
        raise ValueError("problem_type 'regression': a regression head has no class scores; text classification needs labels")
    return HEAD_SIGMOID if problem == "multi_label_classification" or num_labels == 1 else HEAD_SOFTMAX


def longformer_config(config: Dict[str, Any]) -> Tuple[SentenceEncoderConfig, List[int], int]:
    """config.json of a Longformer checkpoint -> (the encoder's config, attention_window per layer, num_labels)"""
    if config.get("model_type") != "longformer":
        raise ValueError(f"model_type {config.get('model_type')!r}: a Longformer config.json is expected")
    if config.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act {config.get('hidden_act')!r}: the encoder block has the erf GELU")
    if config.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"position_embedding_type {config.get('position_embedding_type')!r}: a learned position table is expected")
    depth = int(config["num_hidden_layers"])
    aw = config["attention_window"]
    windows = [int(aw)] * depth if isinstance(aw, int) else [int(a) for a in aw]
    if len(windows) != depth:
        raise ValueError(f"attention_window has {len(windows)} entries for {depth} layers")
    if "id2label" in config:
        num_labels = len(config["id2label"])
    else:
        num_labels = int(config.get("num_labels", 2))
    pad = int(config.get("pad_token_id", 1))
    cfg = SentenceEncoderConfig(vocab=int(config["vocab_size"]), max_position=int(config["max_position_embeddings"]),
                                type_vocab=int(config.get("type_vocab_size", 1)), dim=int(config["hidden_size"]),
                                heads=int(config["num_attention_heads"]), depth=depth, ffn=int(config["intermediate_size"]),
                                ln_eps=float(config.get("layer_norm_eps", 1e-12)), position=0, mlp=0, pool=1, normalize=0,
                                pos_offset=pad + 1, rel_buckets=0, rel_max_distance=0)
    return cfg, windows, num_labels


class TextClassifierModel(BertTextModel):
    """``mhip_berttext`` created through ``mhip_berttext_create_cls``: the windowed encoder + the classification head.
    ``embed_ids_host`` and ``debug_taps_host`` of :class:`BertTextModel` work on it (the <s> row, the per-layer stream)."""

    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], config: SentenceEncoderConfig, windows: Sequence[int],
                 num_labels: int, head_function: int, precision: int = PREC_F16):
        self.cfg, self.precision = config, int(precision)
        self.num_labels, self.head_function, self.windows = int(num_labels), int(head_function), [int(w) for w in windows]
        self._create = "create_cls"
        arr = (C.c_int * max(len(self.windows), 1))(*self.windows)
        full = TextClassifierConfig(ex=config, attention_window=C.cast(arr, C.POINTER(C.c_int)) if self.windows else None,
                                    num_labels=self.num_labels, head_function=self.head_function)
        ModelHandle.__init__(self, ctx, "berttext", self.precision, C.byref(full))
        if state is not None:
            self.load_state({k: v for k, v in state.items() if k.startswith(("longformer.", "classifier."))})

    def classify_ids_host(self, ids, lens) -> Tuple[np.ndarray, np.ndarray]:
        """ids int32 (n, npad), lengths int32 (n,) -> (logits, scores) fp32 (n, num_labels), one model call"""
        ids, lens = self._ids(ids, lens)
        logits = np.empty((ids.shape[0], self.num_labels), np.float32)
        scores = np.empty_like(logits)
        self._call("classify_host", _vp(ids), _vp(lens), ids.shape[0], ids.shape[1], _vp(logits), _vp(scores))
        return logits, scores


# ---- the kernels on host arrays (what tests/test_longformer_gpu.py drives)
def window_attention_host(ctx: Context, precision: int, q, k, v, lens, heads: int, w: int) -> np.ndarray:
    """``attn_window``: q, k, v fp32 (B, npad, heads * 64), q already scaled by 1/8 * log2(e), lens int32 (B,), w the one-sided
    window -> fp32, same shape; row 0 and the rows >= lens[b] mean nothing"""
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    lens = np.ascontiguousarray(lens, np.int32).reshape(-1)
    B, npad, D = q.shape
    if D % heads or k.shape != q.shape or v.shape != q.shape or lens.shape[0] != B:
        raise ValueError(f"q, k, v of one shape (B, npad, heads * head_dim) and B lengths expected, got {q.shape}, {k.shape}, {v.shape}, {lens.shape}")
    out = np.empty_like(q)
    check(ctx.h, ctx.lib.mhip_berttext_attention_window_host(ctx.h, int(precision), _vp(q), _vp(k), _vp(v), _vp(lens), int(w), B, int(heads),
                                                             D // heads, npad, _vp(out)), "mhip_berttext_attention_window_host")
    return out


def global_row_attention_host(ctx: Context, precision: int, qg, kg, vg, lens, heads: int) -> np.ndarray:
    """``attn_global_row``: qg fp32 (B, heads * 64) scaled like q, kg, vg fp32 (B, npad, heads * 64) -> fp32 (B, heads * 64)"""
    qg, kg, vg = (np.ascontiguousarray(a, np.float32) for a in (qg, kg, vg))
    lens = np.ascontiguousarray(lens, np.int32).reshape(-1)
    B, npad, D = kg.shape
    if D != heads * 64 or vg.shape != kg.shape or qg.shape != (B, D) or lens.shape[0] != B:
        raise ValueError(f"qg (B, heads * 64), kg, vg (B, npad, heads * 64) and B lengths expected, got {qg.shape}, {kg.shape}, {vg.shape}, {lens.shape}")
    out = np.empty_like(qg)
    check(ctx.h, ctx.lib.mhip_berttext_attention_global_host(ctx.h, int(precision), _vp(qg), _vp(kg), _vp(vg), _vp(lens), B, int(heads), npad,
                                                             _vp(out)), "mhip_berttext_attention_global_host")
    return out


def cls_head_host(ctx: Context, h0, dense_w, dense_b, out_w, out_b, function: int) -> Tuple[np.ndarray, np.ndarray]:
    """``cls_head``: h0 fp32 (B, D) -> (logits, scores) fp32 (B, L); function HEAD_NONE / HEAD_SOFTMAX / HEAD_SIGMOID"""
    h0, dense_w, dense_b, out_w, out_b = (np.ascontiguousarray(a, np.float32) for a in (h0, dense_w, dense_b, out_w, out_b))
    B, D = h0.shape
    L = out_w.shape[0]
    if dense_w.shape != (D, D) or dense_b.shape != (D,) or out_w.shape != (L, D) or out_b.shape != (L,):
        raise ValueError(f"dense (D, D) / (D,) and out_proj (L, D) / (L,) expected, got {dense_w.shape}, {dense_b.shape}, {out_w.shape}, {out_b.shape}")
    logits = np.empty((B, L), np.float32)
    scores = np.empty_like(logits)
    check(ctx.h, ctx.lib.mhip_berttext_cls_head_host(ctx.h, _vp(h0), _vp(dense_w), _vp(dense_b), _vp(out_w), _vp(out_b), B, D, L, int(function),
                                                     _vp(logits), _vp(scores)), "mhip_berttext_cls_head_host")
    return logits, scores


def top_k_entries(scores: Sequence[float], labels: Dict[int, str], top_k: Optional[int]) -> List[Dict[str, Any]]:
    """the pipeline's result of one text: [{"label", "score"}] sorted by score (ties in label order), the first ``top_k``
    (None: all)"""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    if top_k is not None:
        order = order[:max(int(top_k), 0)]
    return [{"label": labels[i], "score": float(scores[i])} for i in order]


class LongformerTextClassifier:
    """A Longformer sequence-classification model directory on the GPU: tokenizer, weights, length-bucketed calls and the
    pipeline's post-processing.  ``state`` / ``config`` (a state dict under the Hugging Face key names, a ``config.json``
    dictionary) replace the files of the same content; ``tokenizer`` names another directory for ``vocab.json`` / ``merges.txt``."""

    TEXT_CHUNK = 64                        # texts of one model call
    WORKSPACE_BUDGET = 3 << 30             # bytes of workspace one call may lay out

    def __init__(self, model_name_or_path: str, tokenizer: Optional[str] = None, *, state: Optional[Dict[str, np.ndarray]] = None,
                 config: Optional[dict] = None, precision: str = "f16", ctx: Optional[Context] = None):
        if precision not in ("f16", "f32"):
            raise ValueError(f"precision {precision!r}: 'f16' or 'f32'")
        if not os.path.isdir(model_name_or_path):
            raise FileNotFoundError(f"model directory {model_name_or_path!r} does not exist (models are local directories)")
        self.model_dir = model_name_or_path
        tok_dir = tokenizer if tokenizer is not None else model_name_or_path
        self.tokenizer = ByteLevelBPE(os.path.join(tok_dir, "vocab.json"), os.path.join(tok_dir, "merges.txt"))
        if config is None:
            with open(os.path.join(model_name_or_path, "config.json"), encoding="utf-8") as f:
                config = json.load(f)
        self.hf_config = dict(config)
        self.cfg, self.attention_window, self.num_labels = longformer_config(self.hf_config)
        self.head_function = head_function_of(self.hf_config, self.num_labels)
        labels = self.hf_config.get("id2label") or {i: f"LABEL_{i}" for i in range(self.num_labels)}
        self.id2label = {int(k): v for k, v in labels.items()}
        if self.cfg.pos_offset - 1 != self.tokenizer.pad_id:
            raise ValueError(f"config.json pad_token_id {self.cfg.pos_offset - 1} differs from the tokeniser's <pad> id {self.tokenizer.pad_id}")
        self.max_tokens = self.cfg.max_position - self.cfg.pos_offset      # what the position table holds
        self.model_max_length = self._model_max_length(tok_dir)
        self.precision = PREC_F16 if precision == "f16" else PREC_F32
        self._open_model(state, ctx)

    def _model_max_length(self, tok_dir: str) -> int:
        """``model_max_length`` of tokenizer_config.json where it is a sane number, else the position table's"""
        path = os.path.join(tok_dir, "tokenizer_config.json")
        if os.path.isfile(path):
            with open(path, encoding="utf-8") as f:
                said = json.load(f).get("model_max_length")
            if isinstance(said, (int, float)) and 2 <= said < 1 << 30:
                return min(int(said), self.max_tokens)
        return self.max_tokens

    def _open_model(self, state, ctx):
        self.ctx = ctx if ctx is not None else Context(0)
        if state is None:
            state = _load_state(self.model_dir)
        self.model = TextClassifierModel(self.ctx, state, self.cfg, self.attention_window, self.num_labels, self.head_function, self.precision)

    # ---- tokens ---------------------------------------------------------------------------------------------
    def encode(self, text: str, truncation: bool = True) -> List[int]:
        """``<s>`` sub-tokens ``</s>``; ``truncation`` keeps the first ``model_max_length - 2`` sub-tokens (and ``</s>``), without
        it a text past the position table is a ValueError"""
        ids = self.tokenizer.encode(text, self.model_max_length if truncation else None)
        if len(ids) > self.max_tokens:
            raise ValueError(f"a text of {len(ids)} tokens: the position table holds {self.max_tokens}; pass truncation=True")
        return ids

    # ---- model ----------------------------------------------------------------------------------------------
    def _classify_group(self, ids: np.ndarray, lens: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        return self.model.classify_ids_host(ids, lens)

    def _rows_budget(self) -> int:
        per_row = max(self.model.workspace_bytes(1, 64) // 64, 1)
        return int(min(self.WORKSPACE_BUDGET // per_row, 4096 * 128))

    def classify_ids(self, encoded: Sequence[Sequence[int]], chunk: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """id lists -> (logits, scores) fp32 (n, num_labels), in input order: the texts sorted by length and cut into calls that
        share one ``npad``"""
        n = len(encoded)
        logits = np.zeros((n, self.num_labels), np.float32)
        scores = np.zeros_like(logits)
        if n == 0:
            return logits, scores
        groups = plan_text_groups([len(e) for e in encoded], max(int(chunk or self.TEXT_CHUNK), 1), self._rows_budget())
        for npad, members in groups:
            ids, lens = self.tokenizer.pad([encoded[i] for i in members], npad)
            lg, sc = self._classify_group(ids, lens)
            logits[members], scores[members] = lg, sc
        return logits, scores

    def classify_texts(self, texts: Sequence[str], truncation: bool = True, chunk: Optional[int] = None):
        return self.classify_ids([self.encode(t, truncation) for t in texts], chunk)

    def __call__(self, texts: Sequence[str], top_k: Optional[int] = 1, truncation: bool = True,
                 batch_size: Optional[int] = None) -> List[List[Dict[str, Any]]]:
        """``pipeline("text-classification")(texts, top_k=..., truncation=...)``: per text the ``top_k`` entries by score"""
        _, scores = self.classify_texts(texts, truncation, batch_size)
        return [top_k_entries(row, self.id2label, top_k) for row in scores]

    def close(self):
        m = getattr(self, "model", None)
        if m is not None and hasattr(m, "close"):
            m.close()
