"""The page classifier that runs directly on the OCR result: LayoutLMv3 over the page image, the OCR words and their boxes.

reference: ``TransformersDocumentClassifier`` with ``task="text-classification-multimodal"``
(marie/components/document_classifier/transformers.py:41-361), ``scale_bounding_box`` (marie/components/util.py:4-29) and, for
what the reference delegates to the transformers library, ``LayoutLMv3Processor`` / ``LayoutLMv3TokenizerFast`` (words + boxes
-> ids, token boxes, mask) and ``LayoutLMv3ImageProcessor(apply_ocr=False, do_resize=True, resample=BILINEAR)``.

The model runs in HIP (``layoutlmv3.py``; the image resize and normalisation are part of the model call).  The tokeniser runs on
the host, here, without the transformers library: RoBERTa byte-level BPE from ``vocab.json`` / ``merges.txt``.  ``words`` and
``boxes`` are what ``get_words_and_boxes`` (renderer.py) returns for a page.

Unlike the reference, whose "batch" loops page by page, the pages of a batch go through one model call.  There is no CPU path:
``use_gpu=False`` raises.  ``task="text-classification"`` runs a Longformer over the page's words alone (``text_classifier.py``);
other model families under that task, and ``zero-shot-classification``, are not part of this project.
"""
from __future__ import annotations

import json
import os
import unicodedata
from functools import lru_cache
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import PREC_F16, PREC_F32, Context, MarieHipError
from .layoutlmv3 import PIL_BILINEAR

MAX_LENGTH = 512          # predict_document_image: max_length=512, padding="max_length", truncation=True


# ------------------------------------------------------------------------------------------------ tokeniser
@lru_cache()
def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's byte -> printable unicode character table (the alphabet of byte-level BPE vocabularies)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


_GPT2_PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def _split_gpt2_plain(text: str) -> List[str]:
    """The GPT-2 pre-tokenisation pattern on ``str`` predicates (for interpreters without the ``regex`` module): the same
    alternation, tried in the same order at every position."""
    def cls(c):
        if c.isspace():
            return "s"
        k = unicodedata.category(c)[0]
        return "L" if k == "L" else ("N" if k == "N" else "o")

    out, i, n = [], 0, len(text)
    while i < n:
        for c in _CONTRACTIONS:
            if text.startswith(c, i):
                out.append(c)
                i += len(c)
                break
        else:
            j = i + 1 if text[i] == " " and i + 1 < n and cls(text[i + 1]) != "s" else i
            k = cls(text[j])
            if k != "s":                      # " ?" + a run of one class
                e = j
                while e < n and cls(text[e]) == k:
                    e += 1
            else:                             # \s+(?!\S) | \s+
                e = i
                while e < n and cls(text[e]) == "s":
                    e += 1
                if e < n and e - i > 1:
                    e -= 1
            out.append(text[i:e])
            i = e
    return out


try:
    import regex as _regex

    _GPT2_RE = _regex.compile(_GPT2_PATTERN)

    def split_gpt2(text: str) -> List[str]:
        return _GPT2_RE.findall(text)
except ImportError:      # pragma: no cover
    split_gpt2 = _split_gpt2_plain


class ByteLevelBPE:
    """RoBERTa / LayoutLMv3 byte-level BPE as ``LayoutLMv3Tokenizer`` applies it to OCR words: every word is encoded on its own
    with the leading-space marker (``add_prefix_space=True``), and every sub-token carries its word's box."""

    def __init__(self, vocab_file: str, merges_file: str, bos: str = "<s>", eos: str = "</s>", pad: str = "<pad>",
                 unk: str = "<unk>"):
        with open(vocab_file, encoding="utf-8") as f:
            self.vocab: Dict[str, int] = json.load(f)
        with open(merges_file, encoding="utf-8") as f:
            lines = f.read().split("\n")
        if lines and lines[0].startswith("#version"):
            lines = lines[1:]
        self.ranks: Dict[Tuple[str, str], int] = {}
        for ln in lines:
            parts = ln.split()
            if len(parts) == 2:
                self.ranks.setdefault((parts[0], parts[1]), len(self.ranks))
        for name in (bos, eos, pad, unk):
            if name not in self.vocab:
                raise ValueError(f"vocab.json lacks the special token {name}")
        self.bos_id, self.eos_id, self.pad_id, self.unk_id = (self.vocab[t] for t in (bos, eos, pad, unk))
        self._b2u = bytes_to_unicode()
        self._cache: Dict[str, List[int]] = {}
        self._piece_cache: Dict[str, List[int]] = {}      # text_ids: a piece of the GPT-2 split as it stands, no prefix space

    def _bpe(self, token: str) -> List[str]:
        word = list(token)
        while len(word) > 1:
            best, best_rank = None, None
            for pair in zip(word[:-1], word[1:]):
                r = self.ranks.get(pair)
                if r is not None and (best_rank is None or r < best_rank):
                    best, best_rank = pair, r
            if best is None:
                break
            a, b = best
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    merged.append(a + b)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        return word

    def encode_word(self, word: str) -> List[int]:
        """Sub-token ids of one OCR word (no special tokens)."""
        ids = self._cache.get(word)
        if ids is None:
            text = word if word.startswith(" ") else " " + word
            ids = []
            for piece in split_gpt2(text):
                sym = "".join(self._b2u[b] for b in piece.encode("utf-8"))
                ids.extend(self.vocab.get(t, self.unk_id) for t in self._bpe(sym))
            if len(self._cache) < 65536:
                self._cache[word] = ids
        return ids

    # -- whole texts: the ids the sentence encoders take (``RobertaTokenizer`` on a plain string) ---------------------------
    @classmethod
    def from_dir(cls, model_dir) -> Optional["ByteLevelBPE"]:
        """``vocab.json`` + ``merges.txt`` of a model directory; None where it lacks either"""
        if model_dir is None:
            return None
        vocab, merges = os.path.join(model_dir, "vocab.json"), os.path.join(model_dir, "merges.txt")
        return cls(vocab, merges) if os.path.isfile(vocab) and os.path.isfile(merges) else None

    def __len__(self) -> int:
        return len(self.vocab)

    def text_ids(self, text: str) -> List[int]:
        """the sub-token ids of a whole text: the GPT-2 split of the text as it stands (no prefix space), each piece through
        the byte alphabet and the merges.  Special tokens written out in the text are not recognised"""
        ids: List[int] = []
        for piece in split_gpt2(text):
            got = self._piece_cache.get(piece)
            if got is None:
                sym = "".join(self._b2u[b] for b in piece.encode("utf-8"))
                got = [self.vocab.get(t, self.unk_id) for t in self._bpe(sym)]
                if len(self._piece_cache) < 65536:
                    self._piece_cache[piece] = got
            ids.extend(got)
        return ids

    def encode(self, text: str, max_tokens: Optional[int] = None) -> List[int]:
        """``<s>`` sub-tokens ``</s>`` as ids; with ``max_tokens`` the first ``max_tokens - 2`` sub-tokens are kept"""
        ids = self.text_ids(text)
        if max_tokens is not None:
            if max_tokens < 2:
                raise ValueError(f"max_tokens of {max_tokens}: <s> and </s> alone are two")
            ids = ids[:max_tokens - 2]
        return [self.bos_id] + ids + [self.eos_id]

    def pad(self, encoded: Sequence[Sequence[int]], npad: int) -> Tuple[np.ndarray, np.ndarray]:
        """id lists -> (ids int32 (n, npad) filled with ``<pad>``, lengths int32 (n,))"""
        ids = np.full((len(encoded), npad), self.pad_id, np.int32)
        lens = np.empty(len(encoded), np.int32)
        for i, e in enumerate(encoded):
            if len(e) > npad:
                raise ValueError(f"text {i} has {len(e)} tokens, the rows hold {npad}")
            ids[i, :len(e)] = e
            lens[i] = len(e)
        return ids, lens

    def encode_word_offsets(self, word: str) -> Tuple[List[int], List[int]]:
        """Sub-token ids of one OCR word and, per sub-token, the character offset inside the word at which it starts, as
        ``LayoutLMv3TokenizerFast(..., return_offsets_mapping=True)`` reports it (``trim_offsets``: the leading-space marker
        does not count, so a lone marker and the token after it both start at 0; the byte tokens of one character all start
        at that character)."""
        prefixed = not word.startswith(" ")
        text = " " + word if prefixed else word
        ids: List[int] = []
        starts: List[int] = []
        at = 0                                        # character index in ``text`` of the piece
        for piece in split_gpt2(text):
            owner: List[int] = []                     # character index of every byte of the piece
            for ci, ch in enumerate(piece):
                owner.extend([at + ci] * len(ch.encode("utf-8")))
            sym = "".join(self._b2u[b] for b in piece.encode("utf-8"))
            b = 0
            for t in self._bpe(sym):
                first, end = owner[b], owner[b + len(t) - 1] + 1
                while first < end and text[first].isspace():      # trim_offsets
                    first += 1
                starts.append(max(first - (1 if prefixed else 0), 0))
                ids.append(self.vocab.get(t, self.unk_id))
                b += len(t)
            at += len(piece)
        return ids, starts

    def encode_windows(self, words: Sequence[str], boxes: Sequence[Sequence[int]], max_length: int = MAX_LENGTH,
                       stride: int = 128):
        """``LayoutLMv3TokenizerFast(words, boxes=boxes, truncation=True, stride=128, padding="max_length", max_length=512,
        return_overflowing_tokens=True, return_offsets_mapping=True)``: the sub-tokens of a page cut into windows of
        ``max_length - 2`` that advance by ``max_length - 2 - stride``, each wrapped in ``<s>`` ... ``</s>`` and padded.
        -> (input_ids [n][max_length], bbox [n][max_length][4], attention_mask [n][max_length] int32, first [n][max_length]
        bool).  ``first`` is ``offset_mapping[:, 0] == 0``: what the indexer keeps as "not a sub-word" — the first sub-token(s)
        of a word, and every special and padding token."""
        if len(words) != len(boxes):
            raise ValueError("words and boxes must have the same length")
        room = max_length - 2
        if not 0 <= stride < room:
            raise ValueError(f"stride {stride} must lie in [0, {room})")
        ids: List[int] = []
        bbs: List[List[int]] = []
        first: List[bool] = []
        for w, b in zip(words, boxes):
            sub, starts = self.encode_word_offsets(str(w))
            ids.extend(sub)
            bbs.extend([list(b)] * len(sub))
            first.extend(st == 0 for st in starts)
        spans, start = [], 0
        while True:
            end = min(start + room, len(ids))
            spans.append((start, end))
            if end == len(ids):
                break
            start += room - stride
        n = len(spans)
        input_ids = np.full((n, max_length), self.pad_id, np.int32)
        bbox = np.zeros((n, max_length, 4), np.int32)
        mask = np.zeros((n, max_length), np.int32)
        is_first = np.ones((n, max_length), bool)
        for k, (s0, e0) in enumerate(spans):
            m = e0 - s0
            input_ids[k, 0] = self.bos_id
            input_ids[k, 1 + m] = self.eos_id
            mask[k, :m + 2] = 1
            if m:
                input_ids[k, 1:1 + m] = ids[s0:e0]
                bbox[k, 1:1 + m] = np.asarray(bbs[s0:e0], np.int64).reshape(m, 4)
                is_first[k, 1:1 + m] = first[s0:e0]
        return input_ids, bbox, mask, is_first

    def encode_page(self, words: Sequence[str], boxes: Sequence[Sequence[int]], max_length: int = MAX_LENGTH):
        """``LayoutLMv3Tokenizer(words, boxes=boxes, max_length=512, padding="max_length", truncation=True)``:
        (input_ids, bbox, attention_mask) as int32 arrays of max_length (x 4).  ``<s>``, ``</s>`` and ``<pad>`` carry
        [0, 0, 0, 0]; truncation keeps the first max_length - 2 sub-tokens."""
        if len(words) != len(boxes):
            raise ValueError("words and boxes must have the same length")
        ids, bbs = [self.bos_id], [[0, 0, 0, 0]]
        room = max_length - 2
        for w, b in zip(words, boxes):
            if room <= 0:
                break
            sub = self.encode_word(str(w))[:room]
            ids.extend(sub)
            bbs.extend([list(b)] * len(sub))
            room -= len(sub)
        ids.append(self.eos_id)
        bbs.append([0, 0, 0, 0])
        n = len(ids)
        input_ids = np.full((max_length,), self.pad_id, np.int32)
        bbox = np.zeros((max_length, 4), np.int32)
        mask = np.zeros((max_length,), np.int32)
        input_ids[:n] = ids
        bbox[:n] = np.asarray(bbs, np.int64).reshape(n, 4)
        mask[:n] = 1
        return input_ids, bbox, mask


def scale_bounding_box(box: Sequence[int], width_scale: float = 1.0, height_scale: float = 1.0) -> List[int]:
    """marie/components/util.py:24-29."""
    return [int(box[0] * width_scale), int(box[1] * height_scale), int(box[2] * width_scale), int(box[3] * height_scale)]


# ------------------------------------------------------------------------------------------------ classifier
def _load_state(model_dir: str) -> Dict[str, np.ndarray]:
    bin_path = os.path.join(model_dir, "pytorch_model.bin")
    st_path = os.path.join(model_dir, "model.safetensors")
    if os.path.exists(bin_path):
        import torch

        ck = torch.load(bin_path, map_location="cpu", weights_only=True)
        return {k: v.detach().to(torch.float32).numpy() for k, v in ck.items()}
    if os.path.exists(st_path):
        try:
            from safetensors.numpy import load_file
        except ImportError as e:
            raise MarieHipError(f"{st_path} needs the safetensors module, which is not installed") from e
        return {k: np.asarray(v, np.float32) for k, v in load_file(st_path).items()}
    raise FileNotFoundError(f"no pytorch_model.bin or model.safetensors in {model_dir}")


class LayoutLMv3PagePredictor:
    """What the components that run LayoutLMv3 sequence classification page by page share (the document classifier, and
    the document splitter of ``document_splitter.py``): the tokeniser, the weight loader, the model call and the ``predict``
    surface.  A component names the tag its prediction goes under and the Pillow filter of its image processor.

    ``model_name_or_path`` is a local directory with ``config.json``, the weights (``pytorch_model.bin`` or
    ``model.safetensors``) and, unless ``tokenizer`` names another directory, ``vocab.json`` + ``merges.txt``.  ``state`` /
    ``config`` (a state dict under the Hugging Face key names, a ``config.json`` dictionary) replace the files of the same
    content."""

    TAG = "classification"          # documents get tags[TAG]
    RESAMPLE = PIL_BILINEAR         # LayoutLMv3ImageProcessor(resample=...) of the component

    def _setup(self, model_name_or_path: str, tokenizer: Optional[str], use_gpu: bool, batch_size: int,
               id2label: Optional[dict], state: Optional[Dict[str, np.ndarray]], config: Optional[dict], precision: str,
               ctx: Optional[Context]):
        if not use_gpu:
            raise MarieHipError(f"{type(self).__name__} runs on the GPU only: there is no CPU path in this project")
        if precision not in ("f16", "f32"):
            raise ValueError(f"precision {precision!r}: 'f16' or 'f32'")
        if not os.path.isdir(model_name_or_path):
            raise FileNotFoundError(f"model directory {model_name_or_path!r} does not exist (models are local directories)")
        self.batch_size = int(batch_size)
        self.model_dir = model_name_or_path
        tok_dir = tokenizer if tokenizer is not None else model_name_or_path
        self.tokenizer = ByteLevelBPE(os.path.join(tok_dir, "vocab.json"), os.path.join(tok_dir, "merges.txt"))
        if config is None:
            with open(os.path.join(model_name_or_path, "config.json"), encoding="utf-8") as f:
                config = json.load(f)
        self.hf_config = dict(config)
        if id2label is None:
            id2label = self.hf_config.get("id2label")
        if id2label is None:
            id2label = {i: f"LABEL_{i}" for i in range(int(self.hf_config.get("num_labels", 2)))}
        self.id2label = {int(k): v for k, v in id2label.items()}
        self.precision = PREC_F16 if precision == "f16" else PREC_F32
        self._open_model(state, ctx)

    def _open_model(self, state, ctx):
        from .layoutlmv3 import LayoutLMv3Model, config_from_hf

        self.ctx = ctx if ctx is not None else Context(0)
        cfg = config_from_hf(self.hf_config, self.ctx.lib)
        if "id2label" not in self.hf_config and "num_labels" not in self.hf_config:
            cfg.num_labels = len(self.id2label)
        if cfg.pad_id != self.tokenizer.pad_id:
            raise ValueError(f"config.json pad_token_id {cfg.pad_id} differs from the tokeniser's <pad> id {self.tokenizer.pad_id}")
        if state is None:
            state = _load_state(self.model_dir)
        self.model = LayoutLMv3Model(self.ctx, state, cfg, self.precision)
        self.model.set_resample(self.RESAMPLE)

    def _logits(self, pages: List[np.ndarray], ids: np.ndarray, bbox: np.ndarray, mask: np.ndarray) -> np.ndarray:
        """One model call over all pages -> (n, num_labels) fp32."""
        import torch

        from .layoutlmv3 import pack_pages

        packed, descs = pack_pages(pages)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        d_in = torch.from_numpy(packed).cuda()
        logits = self.model.classify_device(d_in.data_ptr(), descs, len(pages), ids, bbox, mask)   # returns after the stream drained
        return logits

    # ---- encoding of one page -------------------------------------------------------------------------------
    def encode(self, image: np.ndarray, words: Sequence[str], boxes: Sequence[Sequence[int]]):
        """Boxes scaled to the 0..1000 grid with int(v * 1000 / size), tokenised, truncated / padded to 512."""
        width, height = image.shape[1], image.shape[0]
        ws, hs = 1000 / width, 1000 / height
        norm = [scale_bounding_box(b, ws, hs) for b in boxes]
        for b in norm:
            if min(b) < 0 or max(b) > 1000:
                raise IndexError("The `bbox` coordinate values should be within 0-1000 range.")
        return self.tokenizer.encode_page(list(words), norm, MAX_LENGTH)

    @staticmethod
    def _frame(image) -> np.ndarray:
        a = np.asarray(image)
        if a.ndim == 2:
            a = np.repeat(a[:, :, None], 3, axis=2)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"page image must be H x W x 3 uint8, got {a.shape} {a.dtype}")
        return np.ascontiguousarray(a)

    def _predict_pages(self, images, words, boxes) -> List[List[Dict[str, Any]]]:
        pages = [self._frame(im) for im in images]
        enc = [self.encode(p, w, b) for p, w, b in zip(pages, words, boxes)]
        ids = np.stack([e[0] for e in enc])
        bbox = np.stack([e[1] for e in enc])
        mask = np.stack([e[2] for e in enc])
        logits = np.asarray(self._logits(pages, ids, bbox, mask), np.float32)
        out = []
        for row in logits:
            z = row.astype(np.float64) - float(row.max())
            p = np.exp(z) / np.exp(z).sum()
            k = int(row.argmax())
            out.append([{"label": self.id2label[k], "score": float(p[k])}])
        return out

    def predict_document_image(self, image: np.ndarray, words: Sequence[str], boxes: Sequence[Sequence[int]],
                               top_k: int = 1) -> List[Dict[str, Any]]:
        """transformers.py:300-361: [{"label", "score"}] of one page (as there, one entry whatever ``top_k``)."""
        return self._predict_pages([image], [words], [boxes])[0]

    def predict(self, documents, words: Optional[List[List[str]]] = None, boxes: Optional[List[List[List[int]]]] = None,
                batch_size: Optional[int] = None):
        """transformers.py:174-298.  ``documents``: objects with ``.tensor`` and a ``.tags`` dict — their
        ``tags["classification"]`` (``tags[TAG]``) is set and they are returned — or plain frames, for which the predictions
        are returned.  Page i is encoded with ``words[i]`` and ``boxes[i]``, whatever the batch size."""
        if batch_size is None:
            batch_size = self.batch_size
        if len(documents) == 0:
            return documents
        assert words is not None and boxes is not None, "words and boxes must be provided for sequence classification"
        assert len(documents) == len(words) == len(boxes), "documents, words and boxes must have the same length"
        plain = not hasattr(documents[0], "tensor")
        frames = [d if plain else d.tensor for d in documents]
        predictions: List[List[Dict[str, Any]]] = []
        for s in range(0, len(frames), max(int(batch_size), 1)):
            e = s + max(int(batch_size), 1)
            predictions.extend(self._predict_pages(frames[s:e], words[s:e], boxes[s:e]))
        formatted = [{"label": p[0]["label"], "score": p[0]["score"], "details": {el["label"]: el["score"] for el in p}}
                     for p in predictions]
        if plain:
            return formatted
        for document, f in zip(documents, formatted):
            document.tags[self.TAG] = f
        return documents

    def close(self):
        m = getattr(self, "model", None)
        if m is not None and hasattr(m, "close"):
            m.close()


class TransformersDocumentClassifier(LayoutLMv3PagePredictor):
    """marie/components/document_classifier/transformers.py:41-361 for ``task="text-classification-multimodal"`` (LayoutLMv3 over
    the page image, words and boxes) and ``task="text-classification"`` (a Longformer over ``" ".join(words)``:
    ``text_classifier.py``); the arguments as on :class:`LayoutLMv3PagePredictor`.  With the text task ``id2label`` renames the
    model's labels as the reference does (``LABEL_n`` -> ``id2label[n]``; labels of another form by their index), and ``boxes`` and
    the page images are accepted and unused."""

    def __init__(self, model_name_or_path: str, tokenizer: Optional[str] = None, use_gpu: bool = True, top_k: int = 1,
                 task: str = "text-classification-multimodal", batch_size: int = 16, id2label: Optional[dict] = None, *,
                 state: Optional[Dict[str, np.ndarray]] = None, config: Optional[dict] = None, precision: str = "f16",
                 ctx: Optional[Context] = None, **kwargs):
        if task == "zero-shot-classification":
            raise NotImplementedError(f"task {task!r}: the reference's own predict raises for it; not built")
        if task not in ("text-classification-multimodal", "text-classification"):
            raise ValueError(f"unknown task {task!r}")
        self.task, self.top_k = task, int(top_k)
        if task == "text-classification":
            self._setup_text(model_name_or_path, tokenizer, use_gpu, batch_size, id2label, state, config, precision, ctx)
        else:
            self._setup(model_name_or_path, tokenizer, use_gpu, batch_size, id2label, state, config, precision, ctx)

    # ---- task="text-classification" ---------------------------------------------------------------------------
    def _setup_text(self, model_name_or_path, tokenizer, use_gpu, batch_size, id2label, state, config, precision, ctx):
        if not use_gpu:
            raise MarieHipError(f"{type(self).__name__} runs on the GPU only: there is no CPU path in this project")
        if not os.path.isdir(model_name_or_path):
            raise FileNotFoundError(f"model directory {model_name_or_path!r} does not exist (models are local directories)")
        if config is None:
            with open(os.path.join(model_name_or_path, "config.json"), encoding="utf-8") as f:
                config = json.load(f)
        model_type = config.get("model_type")
        if model_type != "longformer":
            raise NotImplementedError(f"task 'text-classification' with model_type {model_type!r}: only 'longformer' is built")
        self.batch_size = int(batch_size)
        self.model_dir = model_name_or_path
        self.hf_config = dict(config)
        self.text_model = self._open_text_model(model_name_or_path, tokenizer, state, self.hf_config, precision, ctx)
        self.tokenizer, self.ctx = self.text_model.tokenizer, getattr(self.text_model, "ctx", None)
        self.given_id2label = None if id2label is None else {int(k): v for k, v in id2label.items()}
        self.id2label = self.given_id2label if self.given_id2label is not None else dict(self.text_model.id2label)

    def _open_text_model(self, model_dir, tokenizer, state, config, precision, ctx):
        from .text_classifier import LongformerTextClassifier

        return LongformerTextClassifier(model_dir, tokenizer, state=state, config=config, precision=precision, ctx=ctx)

    def _label(self, label: str) -> str:
        """transformers.py:247-250: ``id2label[int(label.split("_")[1])]``; a label of another form goes by its index"""
        if self.given_id2label is None:
            return label
        parts = label.split("_")
        if len(parts) == 2 and parts[0] == "LABEL" and parts[1].isdigit():
            return self.given_id2label[int(parts[1])]
        index = {v: k for k, v in self.text_model.id2label.items()}
        return self.given_id2label[index[label]]

    def predict_texts(self, texts: Sequence[str], batch_size: Optional[int] = None) -> List[List[Dict[str, Any]]]:
        """per text its own ``top_k`` entries, whatever the batch size (the reference concatenates the entries of a batch)"""
        results = self.text_model(list(texts), top_k=self.top_k, truncation=True, batch_size=batch_size or self.batch_size)
        return [[{"label": self._label(el["label"]), "score": el["score"]} for el in page] for page in results]

    def predict(self, documents, words: Optional[List[List[str]]] = None, boxes: Optional[List[List[List[int]]]] = None,
                batch_size: Optional[int] = None):
        if self.task != "text-classification":
            return super().predict(documents, words, boxes, batch_size)
        if len(documents) == 0:
            return documents
        assert words is not None, "words must be provided for text classification"
        assert len(documents) == len(words), "documents and words must have the same length"
        predictions = self.predict_texts([" ".join(str(w) for w in page) for page in words], batch_size)
        formatted = [{"label": p[0]["label"], "score": p[0]["score"], "details": {el["label"]: el["score"] for el in p}}
                     for p in predictions]
        if not hasattr(documents[0], "tags"):
            return formatted
        for document, f in zip(documents, formatted):
            document.tags[self.TAG] = f
        return documents

    def close(self):
        t = getattr(self, "text_model", None)
        if t is not None:
            t.close()
        super().close()
