"""CLIP image and text embeddings and BERT sentence embeddings on the MI355X: ``OpenAIEmbeddings`` /
``OpenAITransformerEmbeddings`` / ``SentenceTransformerEmbeddings`` / ``JinaEmbeddings`` behind the reference's surface.

Mirrors marie/embeddings/{embeddings_object,base}.py and marie/embeddings/openai/{openai_embeddings,openai_trans_embeddings}.py
for what ``VQNNFTemplateMatcher.score`` takes from them: the image embedding of a 224 x 224 snippet clip, 95 % of the weighted
score.  The vision tower (ViT + projection) runs in HIP (csrc/clip_api.hip, the ``mhip_clipvis_*`` entry points); the image
processor — ``convert("RGB")``, Pillow BICUBIC resize of the shortest edge, centre crop — runs through the Pillow-exact resize
the detector already has, and CLIP's normalisation is part of the patch kernel.

Built: the ViT towers (ViT-B/32, ViT-B/16, any width of 64-wide heads up to 1024) from an OpenAI-scheme (``visual.*``) or a
``transformers``-scheme (``vision_model.*`` + ``visual_projection``) state dict, and the text tower of the same checkpoint
(csrc/cliptext_api.hip, ``mhip_cliptext_*``: causal attention in HIP) with its BPE (clip_tokenizer.py) where the checkpoint holds
one and a vocabulary is at hand: ``get_embeddings(texts, image=None)`` embeds ``" ".join(texts)``.  The ``ModifiedResNet``
towers (RN50, RN101, RN50x4 — the reference's default snippet model) have a loader and a class of their own,
``load_clip_resnet_state`` / ``OpenAIResNetEmbeddings`` (csrc/cliprn_api.hip, ``mhip_cliprn_*``); ``OpenAIEmbeddings`` and
``load_clip_vision_state`` refuse them with ``NotImplementedError`` and name those.  Without a text side ``image=None`` raises
``NotImplementedError``.  Errors raise ``MarieHipError`` (a text longer than the context: ``ValueError``); the reference's
``try/except`` returning an empty ``EmbeddingsObject`` is not restated.

The sentence encoders (marie/embeddings/sentence_transformers/sentence_transformers_embeddings.py, marie/embeddings/jina/
jina_embeddings.py) are at the end of the file: Hugging Face BERT (all-MiniLM-L6-v2) and JinaBERT (ALiBi, GEGLU) with masked mean
or [CLS] pooling in HIP (csrc/berttext_api.hip, ``mhip_berttext_*``), WordPiece on the host (wordpiece_tokenizer.py); and, their
keys renamed onto BERT's (``load_sentence_encoder_state``), MPNet, RoBERTa and DistilBERT models, the byte-level BPE of
document_classifier.py for RoBERTa's vocabulary.  A text
takes its model's own limit, as in the reference: 256 tokens (MiniLM's ``max_seq_length``), 8192 (Jina), never more than the
position table has rows.  Texts of at most 128 tokens run through the attention kernel that holds a text's keys in LDS, longer
ones through the one that streams them; the two never share an encoder call.  A text past the limit raises ``ValueError`` unless
``truncation=True`` cuts it to ``max_tokens`` tokens.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import os
import re
from abc import ABC, abstractmethod
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import (PREC_F16, PREC_F32, STAGE_GUARD, BertTextConfig, ClipResNetConfig, ClipTextConfig, ClipVisConfig, Context,
                   MarieHipError, ModelHandle, SentenceEncoderConfig, check, load)
from .clip_tokenizer import ClipTokenizer
from .document_classifier import ByteLevelBPE
from .wordpiece_tokenizer import WordPieceTokenizer

logger = logging.getLogger(__name__)


class EmbeddingsObject:
    """marie/embeddings/embeddings_object.py"""

    def __init__(self):
        self.embeddings = None
        self.total_tokens = 0


class EmbeddingsBase(ABC):
    """marie/embeddings/base.py"""

    def __init__(self, **kwargs) -> None:
        super().__init__()
        self.logger = logging.getLogger(self.__class__.__name__)

    @abstractmethod
    def get_embeddings(self, texts: List[str], truncation: bool = None, max_length: int = None) -> EmbeddingsObject:
        """the embedding of ``texts`` (or, in the CLIP classes, of ``image``) and its metadata"""

    def get_embeddings_raw(self, texts: List[str], truncation: bool = None, max_length: int = 256):
        return self.get_embeddings(texts, truncation, max_length).embeddings


# ---------------------------------------------------------------------------------------------------- checkpoint -> state
_HF_LAYER = {"self_attn.out_proj": "attn.out_proj", "layer_norm1": "ln_1", "layer_norm2": "ln_2", "mlp.fc1": "mlp.c_fc",
             "mlp.fc2": "mlp.c_proj"}
_HF_TOP = {"vision_model.embeddings.class_embedding": "visual.class_embedding",
           "vision_model.embeddings.patch_embedding.weight": "visual.conv1.weight",
           "vision_model.embeddings.position_embedding.weight": "visual.positional_embedding",
           "vision_model.pre_layrnorm.weight": "visual.ln_pre.weight", "vision_model.pre_layrnorm.bias": "visual.ln_pre.bias",
           "vision_model.post_layernorm.weight": "visual.ln_post.weight",
           "vision_model.post_layernorm.bias": "visual.ln_post.bias"}


def _f32(t) -> np.ndarray:
    """a checkpoint tensor (torch, any float storage — OpenAI checkpoints are fp16 — or array) as a float32 array"""
    if hasattr(t, "detach"):
        t = t.detach().float().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=np.float32)


_HF_TEXT_TOP = {"text_model.embeddings.token_embedding.weight": "token_embedding.weight",
                "text_model.embeddings.position_embedding.weight": "positional_embedding",
                "text_model.final_layer_norm.weight": "ln_final.weight", "text_model.final_layer_norm.bias": "ln_final.bias"}
# a tower of the ``transformers`` scheme: (top-level keys, projection key -> its OpenAI key, layer prefix -> its OpenAI prefix)
_HF_VISION = (_HF_TOP, "visual_projection.weight", "visual.proj", "vision_model", "visual.transformer")
_HF_TEXT = (_HF_TEXT_TOP, "text_projection.weight", "text_projection", "text_model", "transformer")


def _from_transformers(sd: Dict[str, Any], tower=_HF_VISION) -> Dict[str, np.ndarray]:
    """one tower of the ``transformers`` key scheme -> the OpenAI one: q / k / v concatenated into ``in_proj``, the projection
    transposed"""
    top, proj_in, proj_out, hf_prefix, out_prefix = tower
    layer = re.compile(re.escape(hf_prefix) + r"\.encoder\.layers\.(\d+)\.(.+)\.(weight|bias)$")
    out, qkv = {}, {}
    for key, val in sd.items():
        if key in top:
            out[top[key]] = _f32(val)
        elif key == proj_in:
            out[proj_out] = np.ascontiguousarray(_f32(val).T)
        else:
            m = layer.match(key)
            if not m:
                continue                                        # the other tower, logit_scale, position_ids
            n, name, kind = int(m.group(1)), m.group(2), m.group(3)
            if name in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"):
                qkv[(n, kind, name[10])] = _f32(val)
            elif name in _HF_LAYER:
                out[f"{out_prefix}.resblocks.{n}.{_HF_LAYER[name]}.{kind}"] = _f32(val)
    for n, kind in sorted({(n, kind) for n, kind, _ in qkv}):
        parts = [qkv.get((n, kind, p)) for p in "qkv"]
        if any(p is None for p in parts):
            raise MarieHipError(f"CLIP checkpoint: layer {n} lacks one of q_proj / k_proj / v_proj ({kind})")
        out[f"{out_prefix}.resblocks.{n}.attn.in_proj_{kind}"] = np.concatenate(parts, axis=0)
    return out


def load_clip_vision_state(checkpoint: Dict[str, Any]) -> Tuple[Dict[str, np.ndarray], ClipVisConfig]:
    """A ``torch.load``-ed CLIP checkpoint — ``{"model_state_dict": sd}`` or a bare state dict, OpenAI (``visual.*``) or
    ``transformers`` (``vision_model.*``) keys — -> (the vision tower's tensors under the OpenAI keys as float32 arrays, the
    geometry read from their shapes as ``clip.build_model`` reads it).  Text-tower keys are ignored."""
    sd = checkpoint.get("model_state_dict", checkpoint) if isinstance(checkpoint, dict) else None
    if not isinstance(sd, dict) or not sd:
        raise MarieHipError("CLIP checkpoint: expected a state dict or {'model_state_dict': state dict}")
    if any(k.startswith("visual.layer1.") or k.startswith("visual.attnpool.") for k in sd):
        raise NotImplementedError("CLIP checkpoint holds a ModifiedResNet vision tower (RN50 / RN101 / RN50x4 ...): only the "
                                  "ViT towers are built here; load_clip_resnet_state and OpenAIResNetEmbeddings take it")
    if any(k.startswith("vision_model.") for k in sd):
        state = _from_transformers(sd)
    else:
        state = {k: _f32(v) for k, v in sd.items() if k.startswith("visual.")}
    for need in ("visual.conv1.weight", "visual.positional_embedding", "visual.proj",
                 "visual.transformer.resblocks.0.mlp.c_fc.weight"):
        if need not in state:
            raise MarieHipError(f"CLIP checkpoint: no {need} (neither key scheme matches)")
    conv, pos = state["visual.conv1.weight"], state["visual.positional_embedding"]
    cfg = ClipVisConfig()
    cfg.dim, cfg.patch = int(conv.shape[0]), int(conv.shape[-1])
    cfg.depth = len([k for k in state if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    grid = int(round((pos.shape[0] - 1) ** 0.5))
    if grid * grid + 1 != pos.shape[0]:
        raise MarieHipError(f"CLIP checkpoint: {pos.shape[0]} position rows are no square grid plus the class token")
    cfg.image_size = cfg.patch * grid
    cfg.heads = cfg.dim // 64
    cfg.ffn = int(state["visual.transformer.resblocks.0.mlp.c_fc.weight"].shape[0])
    cfg.proj_dim = int(state["visual.proj"].shape[1])
    cfg.ln_eps = 1e-5
    return state, cfg


_TEXT_KEYS = ("token_embedding.weight", "positional_embedding", "text_projection")


def load_clip_text_state(checkpoint: Dict[str, Any]) -> Optional[Tuple[Dict[str, np.ndarray], ClipTextConfig]]:
    """The text tower of a ``torch.load``-ed CLIP checkpoint (either key scheme, as :func:`load_clip_vision_state` takes it) ->
    (its tensors under the OpenAI keys as float32 arrays, the geometry read from their shapes as ``clip.build_model`` reads
    it), or None when the checkpoint holds no text tower."""
    sd = checkpoint.get("model_state_dict", checkpoint) if isinstance(checkpoint, dict) else None
    if not isinstance(sd, dict) or not sd:
        raise MarieHipError("CLIP checkpoint: expected a state dict or {'model_state_dict': state dict}")
    if any(k.startswith("text_model.") for k in sd):
        state = _from_transformers(sd, _HF_TEXT)
    elif "token_embedding.weight" in sd:
        state = {k: _f32(v) for k, v in sd.items()
                 if k in _TEXT_KEYS or k.startswith("transformer.resblocks.") or k.startswith("ln_final.")}
    else:
        return None
    for need in _TEXT_KEYS + ("ln_final.weight", "transformer.resblocks.0.mlp.c_fc.weight"):
        if need not in state:
            raise MarieHipError(f"CLIP checkpoint: the text tower has no {need}")
    tok, pos = state["token_embedding.weight"], state["positional_embedding"]
    cfg = ClipTextConfig()
    cfg.vocab, cfg.dim = int(tok.shape[0]), int(tok.shape[1])
    cfg.context = int(pos.shape[0])
    cfg.heads = cfg.dim // 64
    cfg.depth = len([k for k in state if k.startswith("transformer.resblocks.") and k.endswith(".attn.in_proj_weight")])
    cfg.ffn = int(state["transformer.resblocks.0.mlp.c_fc.weight"].shape[0])
    cfg.proj_dim = int(state["text_projection"].shape[1])
    cfg.ln_eps = 1e-5
    return state, cfg


# geometry of the ModifiedResNet towers ``clip`` publishes: (layers, width, image_size, proj_dim)
CLIP_RESNETS = {"RN50": ((3, 4, 6, 3), 64, 224, 1024), "RN101": ((3, 4, 23, 3), 64, 224, 512),
                "RN50x4": ((4, 6, 10, 6), 80, 288, 640)}
_RN_BN = ("weight", "bias", "running_mean", "running_var")


def clip_resnet_keys(cfg: ClipResNetConfig) -> Dict[str, Tuple[int, ...]]:
    """every tensor the ModifiedResNet tower of ``cfg`` takes -> its shape, in the order ``finalize`` looks them up"""
    w, E, P = cfg.width, cfg.embed_dim, cfg.proj_dim
    keys: Dict[str, Tuple[int, ...]] = {}

    def conv_bn(conv, bn, co, ci, k):
        keys[f"visual.{conv}.weight"] = (co, ci, k, k)
        for name in _RN_BN:
            keys[f"visual.{bn}.{name}"] = (co,)

    conv_bn("conv1", "bn1", w // 2, 3, 3)
    conv_bn("conv2", "bn2", w // 2, w // 2, 3)
    conv_bn("conv3", "bn3", w, w // 2, 3)
    cin = w
    for l in range(4):
        planes = w << l
        for i in range(cfg.layers[l]):
            p = f"layer{l + 1}.{i}."
            conv_bn(p + "conv1", p + "bn1", planes, cin, 1)
            conv_bn(p + "conv2", p + "bn2", planes, planes, 3)
            conv_bn(p + "conv3", p + "bn3", 4 * planes, planes, 1)
            if (i == 0 and l > 0) or cin != 4 * planes:
                conv_bn(p + "downsample.0", p + "downsample.1", 4 * planes, cin, 1)
            cin = 4 * planes
    keys["visual.attnpool.positional_embedding"] = (cfg.grid ** 2 + 1, E)
    for name in "qkv":
        keys[f"visual.attnpool.{name}_proj.weight"], keys[f"visual.attnpool.{name}_proj.bias"] = (E, E), (E,)
    keys["visual.attnpool.c_proj.weight"], keys["visual.attnpool.c_proj.bias"] = (P, E), (P,)
    return keys


def load_clip_resnet_state(checkpoint: Dict[str, Any]) -> Tuple[Dict[str, np.ndarray], ClipResNetConfig]:
    """A ``torch.load``-ed CLIP checkpoint with a ModifiedResNet vision tower — ``{"model_state_dict": sd}`` or a bare state
    dict under the OpenAI keys (``visual.layerL.N.*``, ``visual.attnpool.*``), any float storage — -> (the tower's tensors as
    float32 arrays, the geometry read from their shapes as ``clip.build_model`` reads it).  ``num_batches_tracked`` and the
    text tower's keys are ignored; a missing or misshapen tensor raises ``MarieHipError`` naming it."""
    sd = checkpoint.get("model_state_dict", checkpoint) if isinstance(checkpoint, dict) else None
    if not isinstance(sd, dict) or not sd:
        raise MarieHipError("CLIP checkpoint: expected a state dict or {'model_state_dict': state dict}")
    if "visual.layer1.0.conv1.weight" not in sd or "visual.attnpool.positional_embedding" not in sd:
        if "visual.proj" in sd or any(k.startswith("vision_model.") for k in sd):
            raise MarieHipError("CLIP checkpoint holds a ViT vision tower (visual.proj / vision_model.*): load_clip_vision_state "
                                "and OpenAIEmbeddings take it")
        missing = [k for k in ("visual.layer1.0.conv1.weight", "visual.attnpool.positional_embedding") if k not in sd]
        raise MarieHipError(f"CLIP checkpoint: no {missing[0]} (no ModifiedResNet vision tower under the OpenAI keys)")
    cfg = ClipResNetConfig()
    block = re.compile(r"visual\.layer([1-4])\.(\d+)\.")
    counts = [set(), set(), set(), set()]
    for k in sd:
        m = block.match(k)
        if m:
            counts[int(m.group(1)) - 1].add(int(m.group(2)))
    for l, found in enumerate(counts):
        if not found or found != set(range(len(found))):
            raise MarieHipError(f"CLIP checkpoint: visual.layer{l + 1} has blocks {sorted(found)}, expected 0 .. n - 1")
        cfg.layers[l] = len(found)
    cfg.width = int(sd["visual.layer1.0.conv1.weight"].shape[0])
    pos_rows = int(sd["visual.attnpool.positional_embedding"].shape[0])
    grid = int(round((pos_rows - 1) ** 0.5))
    if grid < 1 or grid * grid + 1 != pos_rows:
        raise MarieHipError(f"CLIP checkpoint: {pos_rows} position rows of the attention pool are no square grid plus the mean token")
    cfg.image_size = 32 * grid
    if "visual.attnpool.c_proj.weight" not in sd:
        raise MarieHipError("CLIP checkpoint: no visual.attnpool.c_proj.weight")
    cfg.proj_dim = int(sd["visual.attnpool.c_proj.weight"].shape[0])
    cfg.bn_eps = 1e-5
    state = {}
    for key, shape in clip_resnet_keys(cfg).items():
        if key not in sd:
            raise MarieHipError(f"CLIP checkpoint: no {key} (a ModifiedResNet of width {cfg.width}, layers {tuple(cfg.layers)})")
        arr = _f32(sd[key])
        if arr.shape != shape:
            raise MarieHipError(f"CLIP checkpoint: {key} has shape {arr.shape}, the geometry read from the checkpoint asks for {shape}")
        state[key] = arr
    return state, cfg


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)


# ---------------------------------------------------------------------------------------------------- the model handle
class ClipVisionModel(ModelHandle):
    """``mhip_clipvis``: the vision tower + projection on a :class:`Context`."""

    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], config: ClipVisConfig, precision: int = PREC_F16):
        self.cfg, self.precision = config, int(precision)
        super().__init__(ctx, "clipvis", self.precision, C.byref(config))
        self.n_tok = (config.image_size // config.patch) ** 2 + 1      # the class token + the patch grid
        if state is not None:
            self.load_state(state)

    def _clips(self, clips) -> np.ndarray:
        S = self.cfg.image_size
        clips = np.ascontiguousarray(clips, np.uint8)
        if clips.ndim == 3:
            clips = clips[None]
        if clips.ndim != 4 or clips.shape[1:] != (S, S, 3) or clips.shape[0] < 1:
            raise ValueError(f"clips of shape (n, {S}, {S}, 3) expected, got {clips.shape}")
        return clips

    def workspace_bytes(self, n: int) -> int:
        return int(self.lib.mhip_clipvis_workspace_bytes(self.h, int(n)))

    def embed_host(self, clips, swap_rb: bool = False) -> np.ndarray:
        """uint8 clips (n, S, S, 3), RGB (or BGR with ``swap_rb``) -> embeddings fp32 (n, proj_dim), one encoder call"""
        clips = self._clips(clips)
        out = np.empty((clips.shape[0], self.cfg.proj_dim), np.float32)
        self._call("embed_host", _vp(clips), clips.shape[0], 1 if swap_rb else 0, _vp(out))
        return out

    def embed_pairs_host(self, clips_bgr, pairs, want_embeddings: bool = False):
        """BGR clips through the encoder once and the cosine of every (a, b) index pair -> fp32 (n_pairs,)
        (, embeddings (n, proj_dim))"""
        clips = self._clips(clips_bgr)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        cos = np.empty(len(pairs), np.float32)
        emb = np.empty((clips.shape[0], self.cfg.proj_dim), np.float32) if want_embeddings else None
        self._call("embed_pairs_host", _vp(clips), clips.shape[0], _vp(pa), _vp(pb), len(pairs), _vp(emb), _vp(cos))
        return (cos, emb) if want_embeddings else cos

    def debug_taps_host(self, clips, swap_rb: bool = False):
        """-> (taps fp32 (depth + 1, n, tokens, dim): the residual stream after the embedding and after every layer,
        embeddings (n, proj_dim))"""
        clips = self._clips(clips)
        n = clips.shape[0]
        taps = np.empty((self.cfg.depth + 1, n, self.n_tok, self.cfg.dim), np.float32)
        emb = np.empty((n, self.cfg.proj_dim), np.float32)
        self._call("debug_taps_host", _vp(clips), n, 1 if swap_rb else 0, _vp(taps), _vp(emb))
        return taps, emb


class ClipResNetModel(ClipVisionModel):
    """``mhip_cliprn``: CLIP's ModifiedResNet tower (stem, four layers of Bottleneck blocks, attention pool) on a
    :class:`Context`.  The entries are :class:`ClipVisionModel`'s; the taps differ."""

    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], config: ClipResNetConfig, precision: int = PREC_F16):
        self.cfg, self.precision = config, int(precision)
        ModelHandle.__init__(self, ctx, "cliprn", self.precision, C.byref(config))
        self.n_tok = config.grid ** 2 + 1      # the mean token + the last map
        if state is not None:
            self.load_state(state)

    def workspace_bytes(self, n: int) -> int:
        return int(self.lib.mhip_cliprn_workspace_bytes(self.h, int(n)))

    def tap_shape(self, i: int) -> Tuple[int, int, int]:
        """(H, W, C) of tap ``i``: 0 the stem after its pool, 1 .. 4 the layers, 5 the embedding"""
        shape = (C.c_int32 * 3)()
        self._call("tap_shape", int(i), shape)
        return tuple(shape)

    def debug_taps_host(self, clips, swap_rb: bool = False):
        """-> ([5 arrays fp32 (n, H, W, C)]: the stem after its pool and the output of every layer, the checkpoint's channel
        counts; embeddings (n, proj_dim))"""
        clips = self._clips(clips)
        n = clips.shape[0]
        shapes = [self.tap_shape(i) for i in range(5)]
        flat = np.empty(n * sum(h * w * c for h, w, c in shapes), np.float32)
        emb = np.empty((n, self.cfg.proj_dim), np.float32)
        self._call("debug_taps_host", _vp(clips), n, 1 if swap_rb else 0, _vp(flat), _vp(emb))
        taps, at = [], 0
        for h, w, c in shapes:
            taps.append(flat[at:at + n * h * w * c].reshape(n, h, w, c))
            at += n * h * w * c
        return taps, emb


class ClipTextModel(ModelHandle):
    """``mhip_cliptext``: the text tower + projection on a :class:`Context`.  Ids come from :class:`ClipTokenizer`."""

    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], config: ClipTextConfig, precision: int = PREC_F16):
        self.cfg, self.precision = config, int(precision)
        super().__init__(ctx, "cliptext", self.precision, C.byref(config))
        if state is not None:
            self.load_state(state)

    @staticmethod
    def _ids(ids, eot) -> Tuple[np.ndarray, np.ndarray]:
        ids, eot = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(eot, np.int32).reshape(-1)
        if ids.ndim != 2 or ids.shape[0] < 1 or eot.shape[0] != ids.shape[0]:
            raise ValueError(f"ids of shape (n, npad) and eot of shape (n,) expected, got {ids.shape} and {eot.shape}")
        return ids, eot

    def workspace_bytes(self, n: int, npad: int) -> int:
        return int(self.lib.mhip_cliptext_workspace_bytes(self.h, int(n), int(npad)))

    def embed_ids_host(self, ids, eot) -> np.ndarray:
        """ids int32 (n, npad), eot int32 (n,) -> embeddings fp32 (n, proj_dim), one tower call"""
        ids, eot = self._ids(ids, eot)
        out = np.empty((ids.shape[0], self.cfg.proj_dim), np.float32)
        self._call("embed_host", _vp(ids), _vp(eot), ids.shape[0], ids.shape[1], _vp(out))
        return out

    def embed_pairs_host(self, ids, eot, pairs, want_embeddings: bool = False):
        """the texts through the tower once and the cosine of every (a, b) index pair -> fp32 (n_pairs,)
        (, embeddings (n, proj_dim))"""
        ids, eot = self._ids(ids, eot)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        cos = np.empty(len(pairs), np.float32)
        emb = np.empty((ids.shape[0], self.cfg.proj_dim), np.float32) if want_embeddings else None
        self._call("embed_pairs_host", _vp(ids), _vp(eot), ids.shape[0], ids.shape[1], _vp(pa), _vp(pb), len(pairs), _vp(cos), _vp(emb))
        return (cos, emb) if want_embeddings else cos

    def debug_taps_host(self, ids, eot):
        """-> (taps fp32 (depth + 1, n, npad, dim): the residual stream after the embedding and after every layer,
        embeddings (n, proj_dim))"""
        ids, eot = self._ids(ids, eot)
        n, npad = ids.shape
        taps = np.empty((self.cfg.depth + 1, n, npad, self.cfg.dim), np.float32)
        emb = np.empty((n, self.cfg.proj_dim), np.float32)
        self._call("debug_taps_host", _vp(ids), _vp(eot), n, npad, _vp(taps), _vp(emb))
        return taps, emb


# ---- the kernels on host arrays (what tests/test_clip_gpu.py and tests/test_cliptext_gpu.py drive)
def text_embed_rows_host(ctx: Context, table, pos, ids) -> np.ndarray:
    """table (vocab, D), pos (npad, D), ids int32 (B, npad) -> h fp32 (B, npad, D) = table[ids] + pos"""
    table, pos = np.ascontiguousarray(table, np.float32), np.ascontiguousarray(pos, np.float32)
    ids = np.ascontiguousarray(ids, np.int32)
    B, npad = ids.shape
    out = np.empty((B, npad, table.shape[1]), np.float32)
    check(ctx.h, ctx.lib.mhip_cliptext_embed_rows_host(ctx.h, _vp(table), _vp(pos), _vp(ids), B, npad, table.shape[0], table.shape[1],
                                                       _vp(out)), "mhip_cliptext_embed_rows_host")
    return out


def causal_attention_host(ctx: Context, precision: int, q, k, v, heads: int) -> np.ndarray:
    """q, k, v fp32 (B, npad, heads * 64), q already scaled by head_dim^-0.5 * log2(e) -> fp32, same shape"""
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    B, npad, D = q.shape
    if D != heads * 64 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"q, k, v of shape (B, npad, {heads * 64}) expected, got {q.shape}, {k.shape}, {v.shape}")
    out = np.empty_like(q)
    check(ctx.h, ctx.lib.mhip_cliptext_attention_host(ctx.h, int(precision), _vp(q), _vp(k), _vp(v), B, int(heads), npad, _vp(out)),
          "mhip_cliptext_attention_host")
    return out


def text_head_host(ctx: Context, h, g, b, proj, row_of, eps: float = 1e-5) -> np.ndarray:
    """h (B, npad, D) (row row_of[i] of block i), LayerNorm g / b (D), proj (D, E) -> fp32 (B, E)"""
    h, g, b, proj = (np.ascontiguousarray(a, np.float32) for a in (h, g, b, proj))
    row_of = np.ascontiguousarray(row_of, np.int32)
    B, npad, D = h.shape
    out = np.empty((B, proj.shape[1]), np.float32)
    check(ctx.h, ctx.lib.mhip_cliptext_head_host(ctx.h, _vp(h), B, npad, D, _vp(g), _vp(b), float(eps), _vp(proj), proj.shape[1],
                                                 _vp(row_of), _vp(out)), "mhip_cliptext_head_host")
    return out


def quick_gelu_host(ctx: Context, precision: int, x) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.empty_like(x)
    check(ctx.h, ctx.lib.mhip_clipvis_quick_gelu_host(ctx.h, int(precision), _vp(x), x.size, _vp(out)), "mhip_clipvis_quick_gelu_host")
    return out


def embed_rows_host(ctx: Context, patches, cls, pos, g, b, eps: float = 1e-5) -> np.ndarray:
    """patches (B, n_tok - 1, D), cls (D), pos (n_tok, D), LayerNorm g / b -> h fp32 (B, roundup(n_tok, 8), D)"""
    patches, cls, pos, g, b = (np.ascontiguousarray(a, np.float32) for a in (patches, cls, pos, g, b))
    B, np_, D = patches.shape
    n_tok = np_ + 1
    out = np.empty((B, (n_tok + 7) // 8 * 8, D), np.float32)
    check(ctx.h, ctx.lib.mhip_clipvis_embed_rows_host(ctx.h, _vp(patches), _vp(cls), _vp(pos), _vp(g), _vp(b), B, n_tok, D,
                                                      float(eps), _vp(out)), "mhip_clipvis_embed_rows_host")
    return out


def head_host(ctx: Context, h, g, b, proj, eps: float = 1e-5) -> np.ndarray:
    """h (B, npad, D) (row 0 of every image), LayerNorm g / b (D), proj (D, E) -> fp32 (B, E)"""
    h, g, b, proj = (np.ascontiguousarray(a, np.float32) for a in (h, g, b, proj))
    B, npad, D = h.shape
    out = np.empty((B, proj.shape[1]), np.float32)
    check(ctx.h, ctx.lib.mhip_clipvis_head_host(ctx.h, _vp(h), B, npad, D, _vp(g), _vp(b), float(eps), _vp(proj), proj.shape[1],
                                                _vp(out)), "mhip_clipvis_head_host")
    return out


def resnet_stem_host(ctx: Context, precision: int, clips, w, scale, bias, swap_rb: bool = False) -> np.ndarray:
    """the ModifiedResNet's first convolution alone: uint8 clips (B, S, S, 3), w (C0, 3, 3, 3), the folded BatchNorm scale / bias
    (C0) -> fp32 (B, S / 2, S / 2, C0) = relu(scale * conv_stride2_pad1(normalised clip) + bias)"""
    clips = np.ascontiguousarray(clips, np.uint8)
    w, scale, bias = (np.ascontiguousarray(a, np.float32) for a in (w, scale, bias))
    B, S = clips.shape[:2]
    if clips.shape != (B, S, S, 3) or w.shape[1:] != (3, 3, 3) or scale.shape != (w.shape[0],) or bias.shape != scale.shape:
        raise ValueError(f"clips (B, S, S, 3), w (C0, 3, 3, 3), scale / bias (C0) expected, got {clips.shape}, {w.shape}, {scale.shape}")
    out = np.empty((B, S // 2, S // 2, w.shape[0]), np.float32)
    check(ctx.h, ctx.lib.mhip_cliprn_stem_host(ctx.h, int(precision), _vp(clips), B, S, 1 if swap_rb else 0, _vp(w), _vp(scale), _vp(bias),
                                               w.shape[0], _vp(out)), "mhip_cliprn_stem_host")
    return out


def avgpool_nhwc_host(ctx: Context, precision: int, x, k: int = 2) -> np.ndarray:
    """x fp32 (B, H, W, C) -> fp32 (B, H / k, W / k, C): the mean of every k x k window"""
    x = np.ascontiguousarray(x, np.float32)
    B, H, W, Cc = x.shape
    out = np.empty((B, H // k, W // k, Cc), np.float32)
    check(ctx.h, ctx.lib.mhip_avgpool_nhwc_host(ctx.h, int(precision), _vp(x), B, H, W, Cc, int(k), _vp(out)), "mhip_avgpool_nhwc_host")
    return out


def resnet_attnpool_host(ctx: Context, precision: int, x, pos, wq, bq, wk, bk, wv, bv, wc, bc) -> np.ndarray:
    """the attention pool alone: x fp32 (B, HW, E) the last map, pos (HW + 1, E), the q / k / v projections (E, E) + (E), c_proj
    (P, E) + (P) -> fp32 (B, P)"""
    x, pos, wq, bq, wk, bk, wv, bv, wc, bc = (np.ascontiguousarray(a, np.float32) for a in (x, pos, wq, bq, wk, bk, wv, bv, wc, bc))
    B, HW, E = x.shape
    P = wc.shape[0]
    if pos.shape != (HW + 1, E) or any(a.shape != (E, E) for a in (wq, wk, wv)) or any(a.shape != (E,) for a in (bq, bk, bv)) or \
            wc.shape != (P, E) or bc.shape != (P,):
        raise ValueError("attention pool: x (B, HW, E), pos (HW + 1, E), projections (E, E) + (E), c_proj (P, E) + (P) expected")
    out = np.empty((B, P), np.float32)
    check(ctx.h, ctx.lib.mhip_cliprn_attnpool_host(ctx.h, int(precision), _vp(x), _vp(pos), _vp(wq), _vp(bq), _vp(wk), _vp(bk), _vp(wv),
                                                   _vp(bv), _vp(wc), _vp(bc), B, HW, E, P, _vp(out)), "mhip_cliprn_attnpool_host")
    return out


def pair_cosine_host(ctx: Context, emb, pairs) -> np.ndarray:
    """emb (n, E) fp32, pairs (n_pairs, 2) of row indices -> fp32 (n_pairs,)"""
    emb = np.ascontiguousarray(emb, np.float32)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    out = np.empty(len(pairs), np.float32)
    check(ctx.h, ctx.lib.mhip_clipvis_pair_cosine_host(ctx.h, _vp(emb), emb.shape[0], emb.shape[1], _vp(pa), _vp(pb), len(pairs),
                                                       _vp(out)), "mhip_clipvis_pair_cosine_host")
    return out


# ---------------------------------------------------------------------------------------------------- preprocessing
def resized_size(width: int, height: int, size: int) -> Tuple[int, int]:
    """(w, h) after the image processor's shortest-edge resize: the short edge becomes ``size``, the long one
    ``int(size * long / short)`` (truncated, not rounded)"""
    short, long = (width, height) if width <= height else (height, width)
    new_long = int(size * long / short)
    return (size, new_long) if width <= height else (new_long, size)


def center_crop_box(width: int, height: int, size: int) -> Tuple[int, int]:
    """(left, top) of the ``size`` x ``size`` centre crop"""
    return (width - size) // 2, (height - size) // 2


# ---------------------------------------------------------------------------------------------------- the embeddings classes
def _device_id(devices) -> int:
    if not devices:
        return 0
    d = devices[0]
    idx = getattr(d, "index", None)
    if idx is None and isinstance(d, str) and ":" in d:
        idx = int(d.split(":")[1])
    return int(idx or 0)


class ClipImageEmbeddings(EmbeddingsBase):
    """What the two CLIP classes share: the tower, the image processor and the batched entries the matcher uses."""

    def __init__(self, model_name_or_path: Union[str, os.PathLike, None] = None, model_version: Optional[str] = None,
                 use_gpu: bool = True, batch_size: int = 16, use_auth_token: Optional[Union[str, bool]] = None,
                 devices: Optional[List[Any]] = None, show_error: Optional[Union[str, bool]] = True, *,
                 state: Optional[Dict[str, Any]] = None, precision: Union[str, int] = "f16", ctx: Optional[Context] = None,
                 text: Optional[bool] = None, tokenizer: Optional[ClipTokenizer] = None, **kwargs):
        """``model_name_or_path``: a model directory holding ``pytorch_model.bin`` (and, for ``OpenAIEmbeddings``,
        ``marie.json``); ``state``: the loaded checkpoint instead (a state dict or ``{"model_state_dict": ...}``).
        ``text``: None builds the text side when the checkpoint holds a text tower and a vocabulary is at hand (``tokenizer``,
        or ``vocab.json`` + ``merges.txt`` / ``bpe_simple_vocab_16e6.txt.gz`` in the model directory); True raises when either
        is missing; False never builds it."""
        super().__init__(**kwargs)
        if not use_gpu:
            raise MarieHipError(f"{type(self).__name__} here is the MI355X path; use_gpu=False has no implementation")
        self.show_error, self.batch_size = show_error, batch_size
        self.model_name_or_path = model_name_or_path
        if state is None:
            state = self._load_checkpoint(model_name_or_path)
        tensors, cfg = self._load_vision(state)
        text_side = self._text_side(state, text, tokenizer, model_name_or_path)      # before any device work
        if isinstance(precision, str):
            if precision not in ("f16", "f32"):
                raise ValueError(f"precision {precision!r}: 'f16' or 'f32'")
            precision = PREC_F16 if precision == "f16" else PREC_F32
        self.ctx = ctx or Context(_device_id(devices))
        self.model = self._make_vision(tensors, cfg, precision)
        self.image_size, self.proj_dim = cfg.image_size, cfg.proj_dim
        self.encoder_calls = 0               # device encoder calls so far
        self.clips_embedded = 0              # clips those calls carried
        self.text_model, self.tokenizer = None, None
        if text_side is not None:
            (text_tensors, text_cfg), self.tokenizer = text_side
            self.text_model = ClipTextModel(self.ctx, text_tensors, text_cfg, precision)
            self.context_length = text_cfg.context
        self.text_encoder_calls = 0          # device text tower calls so far
        self.texts_embedded = 0              # texts those calls carried

    # -- the vision tower: what a subclass with another tower overrides ---------------------------------------------------
    def _load_vision(self, state):
        """the loaded checkpoint -> (tensors, config) of the vision tower; no device work"""
        return load_clip_vision_state(state)

    def _make_vision(self, tensors, cfg, precision: int):
        """the model handle on ``self.ctx``; ``cfg`` carries ``image_size`` and ``proj_dim``"""
        return ClipVisionModel(self.ctx, tensors, cfg, precision)

    def _text_side(self, state, text, tokenizer, model_dir):
        """((tensors, config), tokenizer) of the text side to build, or None"""
        if text is False:
            return None
        loaded = load_clip_text_state(state)
        if loaded is not None and tokenizer is None:
            tokenizer = ClipTokenizer.from_dir(model_dir, loaded[1].context)
        missing = ([] if loaded is not None else ["the checkpoint holds no text tower"]) + \
                  ([] if tokenizer is not None else ["no vocabulary (a tokenizer argument, or vocab.json + merges.txt / "
                                                     "bpe_simple_vocab_16e6.txt.gz in the model directory)"])
        if missing:
            if text:
                raise MarieHipError(f"{type(self).__name__}(text=True): " + "; ".join(missing))
            return None
        if len(tokenizer.encoder) > loaded[1].vocab:
            raise MarieHipError(f"{type(self).__name__}: the vocabulary has {len(tokenizer.encoder)} entries, the token table "
                                f"{loaded[1].vocab} rows")
        return loaded, tokenizer

    def _load_checkpoint(self, path):
        import torch

        if path is None:
            raise MarieHipError(f"{type(self).__name__}: a model directory or a loaded state is required")
        file = os.path.join(path, "pytorch_model.bin") if os.path.isdir(path) else path
        if not os.path.isfile(file):
            raise MarieHipError(f"{type(self).__name__}: no checkpoint at {file}")
        return torch.load(file, map_location="cpu")

    def close(self):
        self.model.close()
        if getattr(self, "text_model", None) is not None:
            self.text_model.close()

    # -- image processor ---------------------------------------------------------------------------------------------
    def preprocess(self, image) -> np.ndarray:
        """``convert("RGB")`` -> BICUBIC resize of the shortest edge to ``image_size`` -> centre crop: the uint8 RGB clip
        (image_size, image_size, 3) the processor would rescale and normalise (that part is the patch kernel's)"""
        return self._resize_crop(np.ascontiguousarray(np.asarray(image.convert("RGB")), np.uint8))

    def _resize_crop(self, rgb: np.ndarray) -> np.ndarray:
        """uint8 (h, w, 3), either channel order -> (image_size, image_size, 3): BICUBIC shortest edge, centre crop"""
        from .dit import pil_resize_rgb

        S = self.image_size
        h, w = rgb.shape[:2]
        if (w, h) != (S, S):
            nw, nh = resized_size(w, h, S)
            if (nw, nh) != (w, h):
                rgb = pil_resize_rgb(self.ctx, rgb, (nh, nw), filter=3)
            left, top = center_crop_box(nw, nh, S)
            rgb = np.ascontiguousarray(rgb[top:top + S, left:left + S])
        return rgb

    # -- the reference's entry ---------------------------------------------------------------------------------------
    def get_embeddings(self, texts: List[str], truncation: bool = None, max_length: int = None, image=None,
                       boxes: List[List[int]] = None, **kwargs) -> EmbeddingsObject:
        """the embedding of ``image``; without one, of ``" ".join(texts)`` (the reference's join).  ``truncation`` cuts a text
        longer than the model's context, as ``clip.tokenize(truncate=True)``; ``max_length`` is not used: the context length
        is the model's"""
        result = EmbeddingsObject()
        if image is None:
            if getattr(self, "text_model", None) is None:
                raise NotImplementedError("get_embeddings without an image needs the CLIP text tower, and this instance has no "
                                          "text side: the checkpoint holds no text tower, or no vocabulary was found")
            result.embeddings = self.embed_texts([" ".join(texts)], truncation=bool(truncation))
            result.total_tokens = -1
            return result
        result.embeddings = self._embed(self.preprocess(image)[None], swap_rb=False)
        result.total_tokens = -1
        return result

    # -- the matcher's entries -----------------------------------------------------------------------------------------
    def _embed(self, clips: np.ndarray, swap_rb: bool) -> np.ndarray:
        self.encoder_calls += 1
        self.clips_embedded += len(clips)
        return self.model.embed_host(clips, swap_rb=swap_rb)

    def embed_clips(self, clips_u8_bgr) -> np.ndarray:
        """BGR uint8 clips (n, image_size, image_size, 3), as the matcher holds them -> fp32 (n, proj_dim), one encoder call"""
        return self._embed(np.ascontiguousarray(clips_u8_bgr, np.uint8), swap_rb=True)

    def cosine_pairs(self, clips_u8_bgr, pairs: Sequence[Tuple[int, int]], want_embeddings: bool = False):
        """the clips through the encoder once, and the cosine of the embeddings of every (a, b) index pair -> fp32 (n_pairs,)
        (, embeddings fp32 (n, proj_dim))"""
        clips = np.ascontiguousarray(clips_u8_bgr, np.uint8)
        self.encoder_calls += 1
        self.clips_embedded += len(clips)
        return self.model.embed_pairs_host(clips, pairs, want_embeddings=want_embeddings)

    # -- the text side ---------------------------------------------------------------------------------------------------
    TEXT_CHUNK = 1024      # texts of one tower call

    def _need_text(self):
        if getattr(self, "text_model", None) is None:
            raise MarieHipError(f"{type(self).__name__}: no text side (the checkpoint holds no text tower, or no vocabulary)")

    def _encode_texts(self, texts: Sequence[str], truncation: bool):
        return self.tokenizer.encode_batch(texts, truncation=truncation, context_length=self.context_length)

    def embed_texts(self, texts: Sequence[str], truncation: bool = False, chunk: Optional[int] = None) -> np.ndarray:
        """-> fp32 (n, proj_dim); chunks of at most ``TEXT_CHUNK`` texts, one tower call per chunk.  A text's embedding does not
        depend on its chunk, bit for bit."""
        self._need_text()
        texts = list(texts)
        chunk = min(int(chunk or self.TEXT_CHUNK), self.TEXT_CHUNK)
        if chunk < 1:
            raise ValueError(f"chunk of {chunk} texts")
        out = np.empty((len(texts), self.text_model.cfg.proj_dim), np.float32)
        for at in range(0, len(texts), chunk):
            ids, eot = self._encode_texts(texts[at:at + chunk], truncation)
            self.text_encoder_calls += 1
            self.texts_embedded += len(ids)
            out[at:at + len(ids)] = self.text_model.embed_ids_host(ids, eot)
        return out

    def text_cosine_pairs(self, texts: Sequence[str], pairs: Sequence[Tuple[int, int]], want_embeddings: bool = False,
                          truncation: bool = False):
        """the cosine of the embeddings of every (a, b) index pair of ``texts`` -> fp32 (n_pairs,) (, embeddings fp32
        (n, proj_dim)).  Duplicate texts are embedded once."""
        self._need_text()
        texts = list(texts)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= len(texts)):
            raise ValueError(f"a pair names a text outside 0 .. {len(texts) - 1}")
        first: Dict[str, int] = {}
        slot = np.array([first.setdefault(t, len(first)) for t in texts], np.int32)
        unique = list(first)
        if len(unique) <= self.TEXT_CHUNK and len(pairs):
            ids, eot = self._encode_texts(unique, truncation)
            self.text_encoder_calls += 1
            self.texts_embedded += len(unique)
            cos, emb = self.text_model.embed_pairs_host(ids, eot, slot[pairs], want_embeddings=True)
        else:
            emb = self.embed_texts(unique, truncation)
            cos = pair_cosine_host(self.ctx, emb, slot[pairs]) if len(pairs) else np.empty(0, np.float32)
        return (cos, emb[slot]) if want_embeddings else cos

    def pair_cosines(self, embeddings, pairs: Sequence[Tuple[int, int]]) -> np.ndarray:
        """the cosine kernel alone on embeddings already at hand, fp32 (n, proj_dim) -> fp32 (n_pairs,)"""
        return pair_cosine_host(self.ctx, embeddings, pairs)


class OpenAIEmbeddings(ClipImageEmbeddings):
    """marie/embeddings/openai/openai_embeddings.py: the architecture is named by the model directory's ``marie.json``."""

    def __init__(self, model_name_or_path=None, *args, architecture: Optional[str] = None, **kwargs):
        if architecture is None and model_name_or_path is not None and os.path.isdir(model_name_or_path):
            config_file = os.path.join(model_name_or_path, "marie.json")
            if not os.path.isfile(config_file):
                raise MarieHipError(f"{model_name_or_path} does not appear to have a file named marie.json")
            with open(config_file, "r", encoding="utf-8") as f:
                config = json.load(f)
            if "architecture" not in config:
                raise ValueError(f"Model config does not contain 'architecture' key: {config}")
            architecture = config["architecture"]
        if architecture is not None and not str(architecture).startswith("ViT-"):
            raise NotImplementedError(f"CLIP architecture {architecture!r}: only the ViT towers are built (ViT-B/32, ViT-B/16) "
                                      "by this class; the ModifiedResNet / attention-pool tower is OpenAIResNetEmbeddings'")
        self.architecture = architecture
        super().__init__(model_name_or_path, *args, **kwargs)


class OpenAITransformerEmbeddings(ClipImageEmbeddings):
    """marie/embeddings/openai/openai_trans_embeddings.py (``transformers.CLIPModel``, openai/clip-vit-base-patch32)"""


class OpenAIResNetEmbeddings(ClipImageEmbeddings):
    """marie/embeddings/openai/openai_embeddings.py on a ModifiedResNet checkpoint (RN50, RN101, RN50x4 — the architecture of
    marie/clip-snippet-rn50x4, the model both template matchers build by default): the tower runs in HIP (csrc/cliprn_api.hip,
    ``mhip_cliprn_*``).  ``OpenAIEmbeddings`` keeps refusing these architectures; hand this object to a matcher as its
    ``embeddings_processor``.  The matchers hold 224 x 224 BGR clips: ``embed_clips`` and ``cosine_pairs`` bring clips of any one
    size to ``image_size`` by :meth:`preprocess`'s rule (for a square clip one Pillow-exact BICUBIC resize), which is what the
    reference's processor does to the matcher's clip in front of RN50x4."""

    CLIP_CHUNK = 128       # clips of one tower call

    def __init__(self, model_name_or_path=None, *args, architecture: Optional[str] = None, **kwargs):
        """``architecture``: None reads ``marie.json`` of the model directory when there is one; a name must start with ``RN``
        and, for RN50 / RN101 / RN50x4, agree with the geometry read from the checkpoint's shapes (``ValueError``)."""
        if architecture is None and model_name_or_path is not None and os.path.isdir(model_name_or_path):
            config_file = os.path.join(model_name_or_path, "marie.json")
            if os.path.isfile(config_file):
                with open(config_file, "r", encoding="utf-8") as f:
                    architecture = json.load(f).get("architecture")
        if architecture is not None and not str(architecture).startswith("RN"):
            raise ValueError(f"CLIP architecture {architecture!r}: OpenAIResNetEmbeddings builds the ModifiedResNet towers (RN50, "
                             "RN101, RN50x4); OpenAIEmbeddings builds the ViT ones")
        self.architecture = architecture
        super().__init__(model_name_or_path, *args, **kwargs)

    def _load_vision(self, state):
        tensors, cfg = load_clip_resnet_state(state)
        known = CLIP_RESNETS.get(str(self.architecture))
        found = (tuple(cfg.layers), cfg.width, cfg.image_size, cfg.proj_dim)
        if known is not None and known != found:
            raise ValueError(f"CLIP architecture {self.architecture!r} is (layers, width, image, proj_dim) = {known}; the "
                             f"checkpoint's shapes say {found}")
        return tensors, cfg

    def _make_vision(self, tensors, cfg, precision: int):
        return ClipResNetModel(self.ctx, tensors, cfg, precision)

    def _text_side(self, state, text, tokenizer, model_dir):
        side = super()._text_side(state, text, tokenizer, model_dir)
        if side is not None and (side[0][1].dim % 64 or side[0][1].dim > 1024):      # what mhip_cliptext_create takes
            if text:
                raise MarieHipError(f"{type(self).__name__}(text=True): the text tower is {side[0][1].dim} wide; the text kernels "
                                    "take a multiple of 64 up to 1024")
            return None
        return side

    # -- the matcher's entries: clips of any one size ----------------------------------------------------------------------
    def _sized(self, clips_u8_bgr) -> np.ndarray:
        clips = np.ascontiguousarray(clips_u8_bgr, np.uint8)
        if clips.ndim == 3:
            clips = clips[None]
        if clips.ndim != 4 or clips.shape[3] != 3 or clips.shape[0] < 1:
            raise ValueError(f"clips of shape (n, h, w, 3) expected, got {clips.shape}")
        S = self.image_size
        if clips.shape[1:3] != (S, S):
            clips = np.stack([self._resize_crop(c) for c in clips])
        return clips

    def _embed(self, clips: np.ndarray, swap_rb: bool) -> np.ndarray:
        out = np.empty((len(clips), self.proj_dim), np.float32)
        for at in range(0, len(clips), self.CLIP_CHUNK):
            out[at:at + self.CLIP_CHUNK] = super()._embed(clips[at:at + self.CLIP_CHUNK], swap_rb)
        return out

    def embed_clips(self, clips_u8_bgr) -> np.ndarray:
        """BGR uint8 clips (n, h, w, 3) of one size -> fp32 (n, proj_dim); one tower call per ``CLIP_CHUNK`` clips"""
        return self._embed(self._sized(clips_u8_bgr), swap_rb=True)

    def cosine_pairs(self, clips_u8_bgr, pairs: Sequence[Tuple[int, int]], want_embeddings: bool = False):
        """the clips through the tower once (per ``CLIP_CHUNK`` clips), and the cosine of the embeddings of every (a, b) index
        pair -> fp32 (n_pairs,) (, embeddings fp32 (n, proj_dim))"""
        clips = self._sized(clips_u8_bgr)
        if len(clips) <= self.CLIP_CHUNK:
            return super().cosine_pairs(clips, pairs, want_embeddings=want_embeddings)
        emb = self._embed(clips, swap_rb=True)
        cos = pair_cosine_host(self.ctx, emb, pairs)
        return (cos, emb) if want_embeddings else cos


# ---------------------------------------------------------------------------------------------------- BERT sentence encoders
BERT_MAX_TOKENS = 128      # the LDS-resident attention's limit ([CLS] and [SEP] included): the routing boundary, past which
                           # a call streams a text's keys (attn_long)
BERT_LONG_MAX_TOKENS = 8192      # tokens of a text: the streamed attention's limit
BERT_MAX_CALL_ROWS = 4096 * 128  # rows (texts x npad) one encoder call lays out at most
POS_ABSOLUTE, POS_ALIBI = 0, 1
MLP_GELU, MLP_GEGLU = 0, 1
POOL_MEAN, POOL_CLS = 0, 1

_BERT_ATTENTION = [("attention.self.query", "dd"), ("attention.self.key", "dd"), ("attention.self.value", "dd"),
                   ("attention.output.dense", "dd"), ("attention.output.LayerNorm", "d")]
_BERT_MLP = {MLP_GELU: [("intermediate.dense", "fd"), ("output.dense", "df"), ("output.LayerNorm", "d")],
             MLP_GEGLU: [("mlp.gated_layers", "2d"), ("mlp.wo", "df"), ("mlp.layernorm", "d")]}


def alibi_slopes(heads: int) -> np.ndarray:
    """the ALiBi slopes of ``heads`` heads as the encoder builds them, fp32 (heads,)"""
    out = np.empty(int(heads), np.float32)
    rc = load().mhip_berttext_alibi_slopes(int(heads), _vp(out))
    if rc:
        raise MarieHipError(f"mhip_berttext_alibi_slopes({heads}) failed ({rc})")
    return out


def bert_text_keys(cfg: BertTextConfig) -> Dict[str, Tuple[int, ...]]:
    """every tensor the encoder of ``cfg`` takes -> its shape, in the order ``finalize`` looks them up"""
    D, F = cfg.dim, cfg.ffn
    dims = {"d": D, "f": F, "2": 2 * F}
    keys = {"embeddings.word_embeddings.weight": (cfg.vocab, D)}
    if cfg.type_vocab:
        keys["embeddings.token_type_embeddings.weight"] = (cfg.type_vocab, D)
    keys.update({"embeddings.LayerNorm.weight": (D,), "embeddings.LayerNorm.bias": (D,)})
    if cfg.position == POS_ABSOLUTE:
        keys["embeddings.position_embeddings.weight"] = (cfg.max_position, D)
    if getattr(cfg, "rel_buckets", 0):      # a SentenceEncoderConfig
        keys["encoder.relative_attention_bias.weight"] = (cfg.rel_buckets, cfg.heads)
    for n in range(cfg.depth):
        for name, shape in _BERT_ATTENTION + _BERT_MLP[cfg.mlp]:
            if len(shape) == 2:
                keys[f"encoder.layer.{n}.{name}.weight"] = (dims[shape[0]], dims[shape[1]])
            else:
                keys[f"encoder.layer.{n}.{name}.weight"] = (D,)
            if name != "mlp.gated_layers":
                keys[f"encoder.layer.{n}.{name}.bias"] = (dims[shape[0]],)
    return keys


def load_bert_text_state(checkpoint: Dict[str, Any], config_json: Dict[str, Any]) -> Tuple[Dict[str, np.ndarray], BertTextConfig]:
    """A loaded BERT checkpoint (a state dict, an optional ``bert.`` prefix on its keys) and its ``config.json`` -> (the
    encoder's tensors as float32 arrays, the geometry).  The scheme is read from both: ``mlp.gated_layers`` keys or
    ``feed_forward_type: geglu`` make the MLP JinaBERT's, ``position_embedding_type: alibi`` (or no position table) drops the
    position rows.  Pooling and normalisation are the embeddings class's to set.  A missing or misshapen tensor raises,
    named."""
    sd = checkpoint.get("model_state_dict", checkpoint) if isinstance(checkpoint, dict) else None
    if not isinstance(sd, dict) or not sd:
        raise MarieHipError("BERT checkpoint: expected a state dict or {'model_state_dict': state dict}")
    sd = {(k[5:] if k.startswith("bert.") else k): v for k, v in sd.items()}
    cfg = BertTextConfig()
    try:
        cfg.vocab, cfg.dim = int(config_json["vocab_size"]), int(config_json["hidden_size"])
        cfg.heads, cfg.depth = int(config_json["num_attention_heads"]), int(config_json["num_hidden_layers"])
        cfg.ffn = int(config_json["intermediate_size"])
    except KeyError as e:
        raise MarieHipError(f"BERT config.json: no {e.args[0]}") from None
    cfg.max_position = int(config_json.get("max_position_embeddings", 512))
    cfg.type_vocab = int(config_json.get("type_vocab_size", 2))
    cfg.ln_eps = float(config_json.get("layer_norm_eps", 1e-12))
    gated = any(k.endswith("mlp.gated_layers.weight") for k in sd)
    ff = str(config_json.get("feed_forward_type", "geglu" if gated else "original"))
    if ff not in ("original", "geglu"):
        raise NotImplementedError(f"BERT config.json: feed_forward_type {ff!r} (original and geglu are built)")
    cfg.mlp = MLP_GEGLU if ff == "geglu" else MLP_GELU
    pe = str(config_json.get("position_embedding_type",
                             "absolute" if "embeddings.position_embeddings.weight" in sd else "alibi"))
    if pe not in ("absolute", "alibi"):
        raise NotImplementedError(f"BERT config.json: position_embedding_type {pe!r} (absolute and alibi are built)")
    cfg.position = POS_ALIBI if pe == "alibi" else POS_ABSOLUTE
    act = str(config_json.get("hidden_act", "gelu"))
    if act != "gelu":
        raise NotImplementedError(f"BERT config.json: hidden_act {act!r} (the erf GELU is built)")
    cfg.pool, cfg.normalize = POOL_MEAN, 0
    state = {}
    for key, shape in bert_text_keys(cfg).items():
        if key not in sd:
            raise MarieHipError(f"BERT checkpoint: no {key} ({'JinaBERT' if cfg.mlp == MLP_GEGLU else 'Hugging Face BERT'} keys, "
                                f"{'no' if cfg.position == POS_ALIBI else 'a'} position table)")
        arr = _f32(sd[key])
        if arr.shape != shape:
            raise MarieHipError(f"BERT checkpoint: {key} has shape {arr.shape}, the configuration asks for {shape}")
        state[key] = arr
    return state, cfg


# ---- the other families: their keys renamed onto BERT's, the differences as configuration
SENTENCE_FAMILIES = ("bert", "mpnet", "roberta", "distilbert")
_MPNET_LAYER = {"attention.attn.q": "attention.self.query", "attention.attn.k": "attention.self.key",
                "attention.attn.v": "attention.self.value", "attention.attn.o": "attention.output.dense",
                "attention.LayerNorm": "attention.output.LayerNorm", "intermediate.dense": "intermediate.dense",
                "output.dense": "output.dense", "output.LayerNorm": "output.LayerNorm"}
_DISTILBERT_LAYER = {"attention.q_lin": "attention.self.query", "attention.k_lin": "attention.self.key",
                     "attention.v_lin": "attention.self.value", "attention.out_lin": "attention.output.dense",
                     "sa_layer_norm": "attention.output.LayerNorm", "ffn.lin1": "intermediate.dense", "ffn.lin2": "output.dense",
                     "output_layer_norm": "output.LayerNorm"}


def _family_names(family: str, cfg: BertTextConfig) -> Dict[str, str]:
    """canonical (BERT) key -> the family's own key, for every tensor the encoder of ``cfg`` takes"""
    names = {}
    for key in bert_text_keys(cfg):
        own = key
        if key.startswith("encoder.layer.") and family in ("mpnet", "distilbert"):
            _, _, n, rest = key.split(".", 3)
            module, leaf = rest.rsplit(".", 1)
            table = _MPNET_LAYER if family == "mpnet" else _DISTILBERT_LAYER
            inverse = {v: k for k, v in table.items()}
            own = f"{'encoder' if family == 'mpnet' else 'transformer'}.layer.{n}.{inverse[module]}.{leaf}"
        names[key] = own
    return names


def sentence_family(sd: Dict[str, Any], config_json: Dict[str, Any]) -> str:
    """``model_type`` of ``config.json``; without one, what the keys say"""
    kind = config_json.get("model_type")
    if kind is not None:
        if kind not in SENTENCE_FAMILIES:
            raise NotImplementedError(f"sentence encoder: model_type {kind!r} is not built ({', '.join(SENTENCE_FAMILIES)} are)")
        return str(kind)
    keys = [k.split(".", 1)[1] if k.split(".", 1)[0] in SENTENCE_FAMILIES and "." in k else k for k in sd]
    if any(k.startswith("transformer.layer.") for k in keys):
        return "distilbert"
    if "encoder.relative_attention_bias.weight" in keys or any(".attention.attn.q." in k for k in keys):
        return "mpnet"
    if any(k.startswith("roberta.") for k in sd):
        return "roberta"
    return "bert"


def load_sentence_encoder_state(checkpoint: Dict[str, Any], config_json: Dict[str, Any]) -> Tuple[Dict[str, np.ndarray], BertTextConfig, str]:
    """A loaded checkpoint of one of ``SENTENCE_FAMILIES`` (an optional ``<family>.`` prefix on its keys) and its
    ``config.json`` -> (the tensors under the BERT names the encoder takes, plus ``encoder.relative_attention_bias.weight``;
    the geometry; the family).  ``bert`` goes through :func:`load_bert_text_state` unchanged.  RoBERTa and MPNet count
    positions from ``pad_token_id + 1``, DistilBERT and MPNet have no token types, MPNet adds its relative attention bias.  A
    missing or misshapen tensor raises, named by the family's own key."""
    sd = checkpoint.get("model_state_dict", checkpoint) if isinstance(checkpoint, dict) else None
    if not isinstance(sd, dict) or not sd:
        raise MarieHipError("sentence encoder checkpoint: expected a state dict or {'model_state_dict': state dict}")
    family = sentence_family(sd, config_json)
    if family == "bert":
        tensors, bert = load_bert_text_state(checkpoint, config_json)
        cfg = SentenceEncoderConfig()      # the same twelve values, zeros behind them
        for field, _ in BertTextConfig._fields_:
            setattr(cfg, field, getattr(bert, field))
        return tensors, cfg, family
    sd = {(k[len(family) + 1:] if k.startswith(family + ".") else k): v for k, v in sd.items()}
    distil = family == "distilbert"
    fields = (dict(vocab="vocab_size", dim="dim", heads="n_heads", depth="n_layers", ffn="hidden_dim") if distil else
              dict(vocab="vocab_size", dim="hidden_size", heads="num_attention_heads", depth="num_hidden_layers", ffn="intermediate_size"))
    cfg = SentenceEncoderConfig()
    try:
        for field, name in fields.items():
            setattr(cfg, field, int(config_json[name]))
    except KeyError as e:
        raise MarieHipError(f"{family} config.json: no {e.args[0]}") from None
    # a field config.json leaves out takes the library's default (RobertaConfig, MPNetConfig, DistilBertConfig)
    cfg.max_position = int(config_json.get("max_position_embeddings", 512))
    cfg.ln_eps = 1e-12 if distil else float(config_json.get("layer_norm_eps", 1e-12))
    cfg.position, cfg.mlp, cfg.pool, cfg.normalize = POS_ABSOLUTE, MLP_GELU, POOL_MEAN, 0
    act = str(config_json.get("activation" if distil else "hidden_act", "gelu"))
    if act != "gelu":
        raise NotImplementedError(f"{family} config.json: activation {act!r} (the erf GELU is built)")
    pe = str(config_json.get("position_embedding_type", "absolute"))
    if pe != "absolute" or config_json.get("sinusoidal_pos_embds") and "embeddings.position_embeddings.weight" not in sd:
        raise NotImplementedError(f"{family} config.json: position embeddings other than a learned table are not built")
    cfg.pos_offset = 0 if distil else int(config_json.get("pad_token_id", 1)) + 1
    cfg.type_vocab = int(config_json.get("type_vocab_size", 2)) if family == "roberta" else 0
    if family == "mpnet":
        cfg.rel_buckets, cfg.rel_max_distance = int(config_json.get("relative_attention_num_buckets", 32)), 128
        if cfg.rel_buckets != 32:      # MPNetEncoder.compute_position_bias buckets with its default of 32, whatever the table's rows
            raise NotImplementedError(f"mpnet config.json: relative_attention_num_buckets {cfg.rel_buckets} (the model buckets into 32)")
    state = {}
    names = _family_names(family, cfg)
    for key, shape in bert_text_keys(cfg).items():
        own = names[key]
        if own not in sd:
            raise MarieHipError(f"{family} checkpoint: no {own}")
        arr = _f32(sd[own])
        if arr.shape != shape:
            raise MarieHipError(f"{family} checkpoint: {own} has shape {arr.shape}, the configuration asks for {shape}")
        state[key] = arr
    return state, cfg, family


def sentence_tokenizer_from_dir(model_dir, family: str):
    """the tokenizer a model directory holds: ``vocab.txt`` -> :class:`WordPieceTokenizer` (with MPNet's special tokens for that
    family, ``do_lower_case`` of ``tokenizer_config.json``), ``vocab.json`` + ``merges.txt`` -> :class:`ByteLevelBPE`.  A
    directory with neither raises, saying what is needed"""
    special = dict(cls_token="<s>", sep_token="</s>", pad_token="<pad>", unk_token="[UNK]", mask_token="<mask>") if family == "mpnet" else {}
    tokenizer = WordPieceTokenizer.from_dir(model_dir, **special) or ByteLevelBPE.from_dir(model_dir)
    if tokenizer is None:
        have = [f for f in ("tokenizer.json", "sentencepiece.bpe.model", "spiece.model", "tokenizer.model")
                if os.path.isfile(os.path.join(model_dir, f))]
        raise MarieHipError(f"no vocab.txt and no vocab.json + merges.txt in {model_dir}"
                            f"{' (only ' + ', '.join(have) + ')' if have else ''}: the WordPiece tokenizer needs vocab.txt, the byte-level "
                            f"BPE vocab.json and merges.txt; tokenizer.json and SentencePiece models are not read")
    return tokenizer


def rel_table(buckets: int, max_distance: int, weight) -> np.ndarray:
    """MPNet's relative attention bias as the encoder folds it, before the log2(e) factor: weight fp32 (buckets, heads) -> fp32
    (heads, 2 * max_distance + 1) over ``query - key`` in ``-max_distance .. max_distance``"""
    weight = np.ascontiguousarray(weight, np.float32)
    if weight.ndim != 2 or weight.shape[0] != buckets:
        raise ValueError(f"weight of shape ({buckets}, heads) expected, got {weight.shape}")
    out = np.empty((weight.shape[1], 2 * int(max_distance) + 1), np.float32)
    rc = load().mhip_berttext_rel_table(int(buckets), int(max_distance), _vp(weight), weight.shape[1], _vp(out))
    if rc:
        raise MarieHipError(f"mhip_berttext_rel_table({buckets}, {max_distance}) failed ({rc}): the bucket must be defined and constant "
                            f"past the distance")
    return out


def read_sentence_model_dir(model_dir) -> Dict[str, Any]:
    """What a sentence-transformers model directory says beyond ``config.json``: ``pooling`` ("mean" / "cls") of
    ``1_Pooling/config.json`` (or of the Pooling module ``modules.json`` names), ``normalize`` (a Normalize module is listed),
    ``max_seq_length`` of ``sentence_bert_config.json``.  Only the keys the directory settles are returned."""
    out: Dict[str, Any] = {}

    def read(*parts):
        path = os.path.join(model_dir, *parts)
        if not os.path.isfile(path):
            return None
        with open(path, "r", encoding="utf-8") as f:
            return json.load(f)

    pooling_dir = "1_Pooling"
    modules = read("modules.json")
    if modules is not None:
        out["normalize"] = any(str(m.get("type", "")).endswith(".Normalize") for m in modules)
        for m in modules:
            if str(m.get("type", "")).endswith(".Pooling"):
                pooling_dir = m.get("path", pooling_dir)
    pooling = read(pooling_dir, "config.json")
    if pooling is not None:
        modes = [k[len("pooling_mode_"):] for k, v in pooling.items() if k.startswith("pooling_mode_") and v is True]
        if modes == ["mean_tokens"]:
            out["pooling"] = "mean"
        elif modes == ["cls_token"]:
            out["pooling"] = "cls"
        else:
            raise NotImplementedError(f"{os.path.join(model_dir, pooling_dir)}: pooling modes {modes} (mean_tokens or cls_token "
                                      "alone are built)")
    sbert = read("sentence_bert_config.json")
    if sbert is not None and sbert.get("max_seq_length") is not None:
        out["max_seq_length"] = int(sbert["max_seq_length"])
    return out


class BertTextModel(ModelHandle):
    """``mhip_berttext``: a BERT sentence encoder + pooling on a :class:`Context`.  Ids come from
    :class:`~marie_icr_amd.wordpiece_tokenizer.WordPieceTokenizer`."""

    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], config: BertTextConfig, precision: int = PREC_F16):
        self.cfg, self.precision = config, int(precision)
        self._create = "create_ex" if isinstance(config, SentenceEncoderConfig) else "create"
        super().__init__(ctx, "berttext", self.precision, C.byref(config))
        if state is not None:
            self.load_state(state)

    def _fn(self, what: str):      # a SentenceEncoderConfig carries three fields more: its own create entry
        return super()._fn(self._create if what == "create" else what)

    @staticmethod
    def _ids(ids, lens) -> Tuple[np.ndarray, np.ndarray]:
        ids, lens = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(lens, np.int32).reshape(-1)
        if ids.ndim != 2 or ids.shape[0] < 1 or lens.shape[0] != ids.shape[0]:
            raise ValueError(f"ids of shape (n, npad) and lengths of shape (n,) expected, got {ids.shape} and {lens.shape}")
        return ids, lens

    def workspace_bytes(self, n: int, npad: int) -> int:
        return int(self.lib.mhip_berttext_workspace_bytes(self.h, int(n), int(npad)))

    def embed_ids_host(self, ids, lens) -> np.ndarray:
        """ids int32 (n, npad), lengths int32 (n,) -> embeddings fp32 (n, dim), one encoder call"""
        ids, lens = self._ids(ids, lens)
        out = np.empty((ids.shape[0], self.cfg.dim), np.float32)
        self._call("embed_host", _vp(ids), _vp(lens), ids.shape[0], ids.shape[1], _vp(out))
        return out

    def embed_pairs_host(self, ids, lens, pairs, want_embeddings: bool = False):
        """the texts through the encoder once and the cosine of every (a, b) index pair -> fp32 (n_pairs,)
        (, embeddings (n, dim))"""
        ids, lens = self._ids(ids, lens)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        cos = np.empty(len(pairs), np.float32)
        emb = np.empty((ids.shape[0], self.cfg.dim), np.float32) if want_embeddings else None
        self._call("embed_pairs_host", _vp(ids), _vp(lens), ids.shape[0], ids.shape[1], _vp(pa), _vp(pb), len(pairs), _vp(cos), _vp(emb))
        return (cos, emb) if want_embeddings else cos

    def debug_taps_host(self, ids, lens):
        """-> (taps fp32 (depth + 1, n, npad, dim): the residual stream after the embedding kernel and after every layer,
        embeddings (n, dim))"""
        ids, lens = self._ids(ids, lens)
        n, npad = ids.shape
        taps = np.empty((self.cfg.depth + 1, n, npad, self.cfg.dim), np.float32)
        emb = np.empty((n, self.cfg.dim), np.float32)
        self._call("debug_taps_host", _vp(ids), _vp(lens), n, npad, _vp(taps), _vp(emb))
        return taps, emb


# ---- the kernels on host arrays (what tests/test_berttext_gpu.py drives)
def _attention_host(entry: str, ctx: Context, precision: int, q, k, v, lens, heads: int, slopes, table=None) -> np.ndarray:
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    lens = np.ascontiguousarray(lens, np.int32).reshape(-1)
    B, npad, D = q.shape
    if D % heads or k.shape != q.shape or v.shape != q.shape or lens.shape[0] != B:
        raise ValueError(f"q, k, v of one shape (B, npad, heads * head_dim) and B lengths expected, got {q.shape}, {k.shape}, "
                         f"{v.shape}, {lens.shape}")
    if slopes is not None:
        slopes = np.ascontiguousarray(slopes, np.float32).reshape(-1)
        if slopes.shape[0] != heads:
            raise ValueError(f"{heads} slopes expected, got {slopes.shape[0]}")
    out = np.empty_like(q)
    if entry.startswith("mhip_berttext_attention_rel"):
        radius = 0
        if table is not None:
            table = np.ascontiguousarray(table, np.float32)
            if table.ndim != 2 or table.shape[0] != heads or table.shape[1] % 2 != 1:
                raise ValueError(f"a table of shape ({heads}, 2 * radius + 1) expected, got {table.shape}")
            radius = table.shape[1] // 2
        check(ctx.h, getattr(ctx.lib, entry)(ctx.h, int(precision), _vp(q), _vp(k), _vp(v), _vp(lens), _vp(table), radius, B,
                                             int(heads), D // heads, npad, _vp(out)), entry)
        return out
    check(ctx.h, getattr(ctx.lib, entry)(ctx.h, int(precision), _vp(q), _vp(k), _vp(v), _vp(lens), _vp(slopes), B,
                                         int(heads), D // heads, npad, _vp(out)), entry)
    return out


def short_attention_host(ctx: Context, precision: int, q, k, v, lens, heads: int, slopes=None) -> np.ndarray:
    """q, k, v fp32 (B, npad, heads * head_dim), q already scaled by head_dim^-0.5 * log2(e), lens int32 (B,), slopes fp32
    (heads,) in the same log2 units or None -> fp32, same shape.  ``attn_short``: npad is at most 128"""
    return _attention_host("mhip_berttext_attention_host", ctx, precision, q, k, v, lens, heads, slopes)


def long_attention_host(ctx: Context, precision: int, q, k, v, lens, heads: int, slopes=None) -> np.ndarray:
    """the same through the streamed kernel (``attn_long``): npad a multiple of 8 up to 8192, 128 rows and fewer included; the
    rows of 64-query blocks that start at or past a sequence's length come back as zeros"""
    return _attention_host("mhip_berttext_attention_long_host", ctx, precision, q, k, v, lens, heads, slopes)


def short_attention_rel_host(ctx: Context, precision: int, q, k, v, lens, heads: int, table=None) -> np.ndarray:
    """``attn_short`` with a relative-distance table in place of the slopes: table fp32 (heads, 2 R + 1) in the log2 units of q,
    the score of (query i, key j) gets ``table[h, clamp(i - j, -R, R) + R]``; None: no term"""
    return _attention_host("mhip_berttext_attention_rel_host", ctx, precision, q, k, v, lens, heads, None, table)


def long_attention_rel_host(ctx: Context, precision: int, q, k, v, lens, heads: int, table=None) -> np.ndarray:
    """the same through the streamed kernel (``attn_long``)"""
    return _attention_host("mhip_berttext_attention_rel_long_host", ctx, precision, q, k, v, lens, heads, None, table)


def bert_embed_rows_ex_host(ctx: Context, word, type0, pos, g, b, ids, eps: float = 1e-12, pos_offset: int = 0) -> np.ndarray:
    """as :func:`bert_embed_rows_host` with type0 (D) or None (no token types) and the position row of token t at
    ``pos_offset + t``: pos (pos_offset + npad, D) or None"""
    word, g, b = (np.ascontiguousarray(a, np.float32) for a in (word, g, b))
    type0 = None if type0 is None else np.ascontiguousarray(type0, np.float32)
    pos = None if pos is None else np.ascontiguousarray(pos, np.float32)
    ids = np.ascontiguousarray(ids, np.int32)
    B, npad = ids.shape
    if pos is not None and pos.shape != (int(pos_offset) + npad, word.shape[1]):
        raise ValueError(f"pos of shape {(int(pos_offset) + npad, word.shape[1])} expected, got {pos.shape}")
    out = np.empty((B, npad, word.shape[1]), np.float32)
    check(ctx.h, ctx.lib.mhip_berttext_embed_rows_ex_host(ctx.h, _vp(word), _vp(type0), _vp(pos), _vp(g), _vp(b), float(eps), _vp(ids),
                                                          B, npad, word.shape[0], word.shape[1], int(pos_offset), _vp(out)),
          "mhip_berttext_embed_rows_ex_host")
    return out


def bert_embed_rows_host(ctx: Context, word, type0, pos, g, b, ids, eps: float = 1e-12) -> np.ndarray:
    """word (vocab, D), type0 (D), pos (npad, D) or None, LayerNorm g / b (D), ids int32 (B, npad) -> h fp32 (B, npad, D)"""
    word, type0, g, b = (np.ascontiguousarray(a, np.float32) for a in (word, type0, g, b))
    pos = None if pos is None else np.ascontiguousarray(pos, np.float32)
    ids = np.ascontiguousarray(ids, np.int32)
    B, npad = ids.shape
    if pos is not None and pos.shape != (npad, word.shape[1]):
        raise ValueError(f"pos of shape {(npad, word.shape[1])} expected, got {pos.shape}")
    out = np.empty((B, npad, word.shape[1]), np.float32)
    check(ctx.h, ctx.lib.mhip_berttext_embed_rows_host(ctx.h, _vp(word), _vp(type0), _vp(pos), _vp(g), _vp(b), float(eps), _vp(ids),
                                                       B, npad, word.shape[0], word.shape[1], _vp(out)),
          "mhip_berttext_embed_rows_host")
    return out


def row_layernorm_host(ctx: Context, precision: int, x, g, b, eps: float, want_h: bool = True, want_ht: bool = True,
                       in_place: bool = False, x_f16: bool = False, x_lo=None):
    """The row LayerNorm every tower shares (csrc/row_ops.hip): x fp32 (rows, D), g / b (D) -> (h, ht), each None unless asked
    for: h the fp32 rows, ht their copy in the precision's element type (widened).  Both are FLAT and STAGE_GUARD elements longer
    than rows * D: the tail comes back as the 0xff fill unless the kernel wrote past its end.  in_place: h and x share one
    device buffer.  x_f16: x is narrowed to an f16 stream (f16 mode only), x_lo its low plane or None"""
    x, g, b = (np.ascontiguousarray(a, np.float32) for a in (x, g, b))
    x_lo = None if x_lo is None else np.ascontiguousarray(x_lo, np.float32)
    rows, D = x.shape
    h = np.zeros(rows * D + STAGE_GUARD, np.float32) if want_h else None
    ht = np.zeros(rows * D + STAGE_GUARD, np.float32) if want_ht else None
    check(ctx.h, ctx.lib.mhip_row_layernorm_host(ctx.h, int(precision), _vp(x), int(x_f16), _vp(x_lo), _vp(g), _vp(b), rows, D,
                                                 float(eps), int(in_place), _vp(h), _vp(ht)), "mhip_row_layernorm_host")
    return h, ht


def geglu_host(ctx: Context, precision: int, x) -> np.ndarray:
    """x fp32 (R, 2 F) -> fp32 (R, F) = gelu(x[:, :F]) * x[:, F:]"""
    x = np.ascontiguousarray(x, np.float32)
    R, F2 = x.shape
    out = np.empty((R, F2 // 2), np.float32)
    check(ctx.h, ctx.lib.mhip_berttext_geglu_host(ctx.h, int(precision), _vp(x), R, F2 // 2, _vp(out)), "mhip_berttext_geglu_host")
    return out


def bert_pool_host(ctx: Context, h, lens, mode: int = POOL_MEAN, normalize: bool = False) -> np.ndarray:
    """h fp32 (B, npad, D), lens int32 (B,) -> fp32 (B, D)"""
    h = np.ascontiguousarray(h, np.float32)
    lens = np.ascontiguousarray(lens, np.int32).reshape(-1)
    B, npad, D = h.shape
    out = np.empty((B, D), np.float32)
    check(ctx.h, ctx.lib.mhip_berttext_pool_host(ctx.h, _vp(h), _vp(lens), B, npad, D, int(mode), 1 if normalize else 0, _vp(out)),
          "mhip_berttext_pool_host")
    return out


def plan_text_groups(lengths: Sequence[int], max_group: int, rows_budget: Optional[int] = None, *,
                     boundary: Optional[int] = None) -> List[Tuple[int, List[int]]]:
    """The calls of ``embed_texts``: the texts sorted by token count (ties in input order) and cut into groups of at most
    ``max_group`` texts — and, with ``rows_budget``, of at most that many rows — that share one ``npad``, the longest of the
    group rounded up to 8 -> [(npad, [input indices])].  With ``boundary`` no group holds both a text of at most ``boundary``
    tokens and a longer one."""
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    groups: List[Tuple[int, List[int]]] = []
    at = 0
    while at < len(order):
        end = min(at + max_group, len(order))
        if boundary is not None and lengths[order[at]] <= boundary:
            while lengths[order[end - 1]] > boundary:      # sorted: the group's start is on the short side, cut where that ends
                end -= 1
        npad = (lengths[order[end - 1]] + 7) // 8 * 8
        # a shorter group of the same start never needs more rows a text
        while rows_budget is not None and end - at > 1 and (end - at) * npad > rows_budget:
            end -= 1
            npad = (lengths[order[end - 1]] + 7) // 8 * 8
        groups.append((npad, order[at:end]))
        at = end
    return groups


class BertTextEmbeddings(EmbeddingsBase):
    """What the two sentence-embedding classes share: the encoder, the tokenizer, the length-bucketed batching and the
    entries ``MetaTemplateMatcher`` uses (``text_model``, ``embed_texts``, ``pair_cosines``)."""

    POOLING, NORMALIZE = "mean", False       # what a directory without modules.json / 1_Pooling gets
    MAX_LENGTH: Optional[int] = None         # max_seq_length without a sentence_bert_config.json: the position table's
    TEXT_CHUNK = 1024                        # texts of one encoder call
    WORKSPACE_BUDGET = 1 << 30               # bytes of workspace one call may lay out

    def __init__(self, model_name_or_path: Union[str, os.PathLike, None] = None, model_version: Optional[str] = None,
                 use_gpu: bool = True, batch_size: int = 4, use_auth_token: Optional[Union[str, bool]] = None,
                 devices: Optional[List[Any]] = None, show_error: Optional[Union[str, bool]] = True, *,
                 state: Optional[Dict[str, Any]] = None, config: Optional[Dict[str, Any]] = None,
                 tokenizer: Union[WordPieceTokenizer, ByteLevelBPE, None] = None, precision: Union[str, int] = "f16",
                 ctx: Optional[Context] = None, pooling: Optional[str] = None, normalize: Optional[bool] = None,
                 max_seq_length: Optional[int] = None, **kwargs):
        """``model_name_or_path``: a model directory of a BERT, MPNet, RoBERTa or DistilBERT sentence encoder holding
        ``config.json``, ``model.safetensors`` or ``pytorch_model.bin``, ``vocab.txt`` (WordPiece) or ``vocab.json`` + ``merges.txt``
        (byte-level BPE) and, optionally, ``modules.json``, ``1_Pooling/config.json`` and ``sentence_bert_config.json``.
        ``state`` / ``config`` / ``tokenizer``: the loaded checkpoint, the ``config.json`` dict and the tokenizer instead.
        ``pooling`` ("mean" / "cls"), ``normalize`` and ``max_seq_length`` override what the directory (or the class) says."""
        super().__init__(**kwargs)
        if not use_gpu:
            raise MarieHipError(f"{type(self).__name__} here is the MI355X path; use_gpu=False has no implementation")
        self.show_error, self.batch_size = show_error, batch_size
        self.model_name_or_path = model_name_or_path
        said: Dict[str, Any] = {}
        if state is None or config is None or tokenizer is None:
            if model_name_or_path is None or not os.path.isdir(model_name_or_path):
                raise MarieHipError(f"{type(self).__name__}: a model directory, or state, config and tokenizer, is required")
        if model_name_or_path is not None and os.path.isdir(model_name_or_path):
            said = read_sentence_model_dir(model_name_or_path)
        if config is None:
            config = self._load_config(model_name_or_path)
        if state is None:
            state = self._load_checkpoint(model_name_or_path)
        tensors, cfg, family = load_sentence_encoder_state(state, config)      # before any device work
        if tokenizer is None:
            if family == "bert":
                tokenizer = WordPieceTokenizer.from_dir(model_name_or_path)
                if tokenizer is None:
                    raise MarieHipError(f"{type(self).__name__}: no vocab.txt in {model_name_or_path}")
            else:
                tokenizer = sentence_tokenizer_from_dir(model_name_or_path, family)
        self.family = family
        if len(tokenizer) > cfg.vocab:
            raise MarieHipError(f"{type(self).__name__}: the vocabulary has {len(tokenizer)} entries, the word table {cfg.vocab} rows")
        pooling = pooling or said.get("pooling", self.POOLING)
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling {pooling!r}: 'mean' or 'cls'")
        normalize = said.get("normalize", self.NORMALIZE) if normalize is None else normalize
        cfg.pool, cfg.normalize = (POOL_CLS if pooling == "cls" else POOL_MEAN), (1 if normalize else 0)
        self.pooling, self.normalize = pooling, bool(normalize)
        limit = max_seq_length or said.get("max_seq_length") or self.MAX_LENGTH
        if cfg.position == POS_ABSOLUTE:
            limit = min(limit or cfg.max_position - cfg.pos_offset, cfg.max_position - cfg.pos_offset)
        self.max_seq_length = limit                                      # the model's own limit (None: none)
        self.max_tokens = min(limit or BERT_LONG_MAX_TOKENS, BERT_LONG_MAX_TOKENS)   # this build's
        if isinstance(precision, str):
            if precision not in ("f16", "f32"):
                raise ValueError(f"precision {precision!r}: 'f16' or 'f32'")
            precision = PREC_F16 if precision == "f16" else PREC_F32
        self.tokenizer = tokenizer
        self.ctx = ctx or Context(_device_id(devices))
        self.text_model = BertTextModel(self.ctx, tensors, cfg, precision)
        self.dim = cfg.dim
        self.text_encoder_calls = 0          # device encoder calls so far
        self.texts_embedded = 0              # texts those calls carried

    def _load_config(self, path):
        file = os.path.join(path, "config.json")
        if not os.path.isfile(file):
            raise MarieHipError(f"{type(self).__name__}: no config.json in {path}")
        with open(file, "r", encoding="utf-8") as f:
            return json.load(f)

    def _load_checkpoint(self, path):
        file = os.path.join(path, "model.safetensors")
        if os.path.isfile(file):
            from safetensors.numpy import load_file

            return load_file(file)
        file = os.path.join(path, "pytorch_model.bin")
        if os.path.isfile(file):
            import torch

            return torch.load(file, map_location="cpu")
        raise MarieHipError(f"{type(self).__name__}: neither model.safetensors nor pytorch_model.bin in {path}")

    def close(self):
        if getattr(self, "text_model", None) is not None:
            self.text_model.close()

    # -- tokens ----------------------------------------------------------------------------------------------------------
    def encode_texts(self, texts: Sequence[str], truncation: bool = False) -> List[List[int]]:
        """``[CLS]`` .. ``[SEP]`` ids of every text; more than ``max_tokens`` of them raise ``ValueError`` unless ``truncation``"""
        out = []
        for i, text in enumerate(texts):
            ids = self.tokenizer.encode(text, self.max_tokens if truncation else None)
            if len(ids) > self.max_tokens:
                raise ValueError(f"text {i} is too long: {len(ids)} tokens, the model takes at most {self.max_tokens} "
                                 f"(truncation=True cuts it)")
            out.append(ids)
        return out

    def _groups(self, lengths: Sequence[int], chunk: Optional[int]):
        chunk = min(int(chunk or self.TEXT_CHUNK), self.TEXT_CHUNK)
        if chunk < 1:
            raise ValueError(f"chunk of {chunk} texts")
        probe = min(BERT_MAX_TOKENS, (self.max_tokens + 7) // 8 * 8)
        per_row = self.text_model.workspace_bytes(8, probe) // (8 * probe)      # the workspace grows with the rows
        # at least one text of max_tokens; a text of at most BERT_MAX_TOKENS tokens never shares a call with a longer one, so it
        # always runs through attn_short and its embedding does not depend on what it is embedded with
        rows = max(self.WORKSPACE_BUDGET // max(per_row, 1), (self.max_tokens + 7) // 8 * 8)
        return plan_text_groups(lengths, chunk, min(rows, BERT_MAX_CALL_ROWS), boundary=BERT_MAX_TOKENS)

    # -- the matcher's entries -------------------------------------------------------------------------------------------
    def embed_texts(self, texts: Sequence[str], truncation: bool = False, chunk: Optional[int] = None) -> np.ndarray:
        """-> fp32 (n, dim), rows in input order.  The texts are sorted by token count and embedded in groups that share one
        ``npad``; a text's embedding does not depend on its group, bit for bit."""
        encoded = self.encode_texts(list(texts), truncation)
        out = np.empty((len(encoded), self.dim), np.float32)
        for npad, members in self._groups([len(e) for e in encoded], chunk):
            ids, lens = self.tokenizer.pad([encoded[i] for i in members], npad)
            self.text_encoder_calls += 1
            self.texts_embedded += len(members)
            out[members] = self.text_model.embed_ids_host(ids, lens)
        return out

    def text_cosine_pairs(self, texts: Sequence[str], pairs: Sequence[Tuple[int, int]], want_embeddings: bool = False,
                          truncation: bool = False):
        """the cosine of the embeddings of every (a, b) index pair of ``texts`` -> fp32 (n_pairs,) (, embeddings fp32
        (n, dim)).  Duplicate texts are embedded once."""
        texts = list(texts)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= len(texts)):
            raise ValueError(f"a pair names a text outside 0 .. {len(texts) - 1}")
        first: Dict[str, int] = {}
        slot = np.array([first.setdefault(t, len(first)) for t in texts], np.int32)
        emb = self.embed_texts(list(first), truncation)
        cos = pair_cosine_host(self.ctx, emb, slot[pairs]) if len(pairs) else np.empty(0, np.float32)
        return (cos, emb[slot]) if want_embeddings else cos

    def pair_cosines(self, embeddings, pairs: Sequence[Tuple[int, int]]) -> np.ndarray:
        """the cosine kernel alone on embeddings already at hand, fp32 (n, dim) -> fp32 (n_pairs,)"""
        return pair_cosine_host(self.ctx, embeddings, pairs)

    # -- the reference's entry ---------------------------------------------------------------------------------------------
    TOTAL_TOKENS_IS_WIDTH = False

    def get_embeddings(self, texts: List[str], truncation: bool = None, max_length: int = None) -> EmbeddingsObject:
        """one embedding per text, fp32 (n, dim), as the reference's ``encode``.  ``max_length`` is not used: the limit is
        ``max_tokens``"""
        result = EmbeddingsObject()
        result.embeddings = self.embed_texts(texts, truncation=bool(truncation))
        result.total_tokens = len(result.embeddings[0]) if self.TOTAL_TOKENS_IS_WIDTH and len(result.embeddings) else -1
        return result


class SentenceTransformerEmbeddings(BertTextEmbeddings):
    """marie/embeddings/sentence_transformers/sentence_transformers_embeddings.py (``SentenceTransformer``,
    sentence-transformers/all-MiniLM-L6-v2: mean pooling, Normalize, 256 tokens).  ``total_tokens`` is the embedding width,
    the reference's ``len(embeddings[0])``.  ``SentenceTransformer.encode`` always truncates to ``max_seq_length``; here a text
    past ``max_tokens`` raises unless ``truncation=True``."""

    POOLING, NORMALIZE, MAX_LENGTH = "mean", True, 256
    TOTAL_TOKENS_IS_WIDTH = True


class JinaEmbeddings(BertTextEmbeddings):
    """marie/embeddings/jina/jina_embeddings.py (``AutoModel(...).encode``, jinaai/jina-embeddings-v2-base-en: mean pooling, no
    normalisation).  ``total_tokens`` is -1, as there."""

    POOLING, NORMALIZE, MAX_LENGTH = "mean", False, None
