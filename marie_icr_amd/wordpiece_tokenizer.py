"""BERT's WordPiece tokenizer on the host: the ids :class:`~marie_icr_amd.embeddings.BertTextModel` takes.

Restates transformers/models/bert/tokenization_bert.py (``BasicTokenizer`` + ``WordpieceTokenizer`` behind ``BertTokenizer``):
control characters are dropped and white space becomes a blank, CJK ideographs are padded with blanks, a word is lower-cased and
its accents stripped (NFD, category Mn) where the model is uncased, punctuation is split into tokens of its own, the special
tokens are taken out first and left alone, and every word is cut greedily into the longest vocabulary pieces, ``##`` marking a
continuation; a word of more than 100 characters, or one with a stretch no piece covers, is ``[UNK]``.
"""
from __future__ import annotations

import json
import os
import re
import unicodedata
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_CHARS_PER_WORD = 100
WORD_CACHE_ENTRIES = 1 << 16      # blank-separated words whose ids are remembered


def _is_whitespace(ch: str) -> bool:
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch: str) -> bool:
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_punctuation(ch: str) -> bool:
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:      # ASCII non-letters count, "^", "$" and "`" too
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F or
            0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


class WordPieceTokenizer:
    def __init__(self, vocab: Sequence[str], do_lower_case: bool = True, unk_token: str = "[UNK]", cls_token: str = "[CLS]",
                 sep_token: str = "[SEP]", pad_token: str = "[PAD]", mask_token: str = "[MASK]"):
        self.vocab: Dict[str, int] = {tok: i for i, tok in enumerate(vocab)}
        self.do_lower_case = bool(do_lower_case)
        for tok in (unk_token, cls_token, sep_token, pad_token):
            if tok not in self.vocab:
                raise ValueError(f"the vocabulary has no {tok}")
        self.unk_token = unk_token
        self.unk_id, self.cls_id = self.vocab[unk_token], self.vocab[cls_token]
        self.sep_id, self.pad_id = self.vocab[sep_token], self.vocab[pad_token]
        # BERT's names, and the family's own where they differ (MPNet: <s>, </s>, <pad>, [UNK], <mask>)
        self.never_split = frozenset(t for t in (unk_token, sep_token, pad_token, cls_token, mask_token) if t in self.vocab)
        self._word_ids: Dict[str, List[int]] = {}
        self._specials = re.compile("(" + "|".join(re.escape(t) for t in sorted(self.never_split, key=len, reverse=True)) + ")")

    @classmethod
    def from_dir(cls, model_dir, **special_tokens) -> Optional["WordPieceTokenizer"]:
        """``vocab.txt`` (one piece a line) and ``do_lower_case`` of ``tokenizer_config.json`` (default true); None where the
        directory holds no ``vocab.txt``.  ``special_tokens``: ``unk_token`` .. ``mask_token`` where they are not BERT's"""
        if model_dir is None or not os.path.isfile(os.path.join(model_dir, "vocab.txt")):
            return None
        with open(os.path.join(model_dir, "vocab.txt"), "r", encoding="utf-8") as f:
            vocab = [line.rstrip("\n") for line in f]
        while vocab and vocab[-1] == "":
            vocab.pop()
        lower = True
        config = os.path.join(model_dir, "tokenizer_config.json")
        if os.path.isfile(config):
            with open(config, "r", encoding="utf-8") as f:
                lower = bool(json.load(f).get("do_lower_case", True))
        return cls(vocab, do_lower_case=lower, **special_tokens)

    def __len__(self) -> int:
        return len(self.vocab)

    # -- BasicTokenizer ------------------------------------------------------------------------------------------------
    def basic_tokens(self, text: str) -> List[str]:
        chars = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                chars.append(" ")
            elif _is_cjk(cp):
                chars.append(" " + ch + " ")
            else:
                chars.append(ch)
        out: List[str] = []
        for word in unicodedata.normalize("NFC", "".join(chars)).split():
            if self.do_lower_case:
                word = "".join(c for c in unicodedata.normalize("NFD", word.lower()) if unicodedata.category(c) != "Mn")
            piece = ""
            for ch in word:
                if _is_punctuation(ch):
                    if piece:
                        out.append(piece)
                    out.append(ch)
                    piece = ""
                else:
                    piece += ch
            if piece:
                out.append(piece)
        return out

    # -- WordPiece -------------------------------------------------------------------------------------------------------
    def word_pieces(self, word: str) -> List[str]:
        if len(word) > MAX_CHARS_PER_WORD:
            return [self.unk_token]
        pieces, start = [], 0
        while start < len(word):
            end = len(word)
            while end > start:
                sub = word[start:end] if start == 0 else "##" + word[start:end]
                if sub in self.vocab:
                    break
                end -= 1
            if end == start:
                return [self.unk_token]
            pieces.append(sub)
            start = end
        return pieces

    def tokenize(self, text: str) -> List[str]:
        """the pieces of ``text``; a special token is taken out wherever it stands, also inside a word, as ``transformers`` does"""
        out: List[str] = []
        for part in self._specials.split(text):
            if part in self.never_split:
                out.append(part)
                continue
            for word in self.basic_tokens(part):
                out.extend(self.word_pieces(word))
        return out

    def piece_ids(self, text: str) -> List[int]:
        """the ids of ``tokenize(text)``.  Printable ASCII — what OCR words mostly are — is cut at its blanks and every word's ids
        are remembered: each step of ``tokenize`` works inside one blank-separated word"""
        if not (text.isascii() and text.isprintable()):
            return [self.vocab[p] for p in self.tokenize(text)]
        out: List[int] = []
        cache = self._word_ids
        for word in text.split(" "):
            ids = cache.get(word)
            if ids is None:
                if len(cache) >= WORD_CACHE_ENTRIES:
                    cache.clear()
                ids = cache[word] = [self.vocab[p] for p in self.tokenize(word)]
            out.extend(ids)
        return out

    def encode(self, text: str, max_tokens: Optional[int] = None) -> List[int]:
        """``[CLS]`` pieces ``[SEP]`` as ids; with ``max_tokens`` the first ``max_tokens - 2`` pieces are kept"""
        ids = self.piece_ids(text)
        if max_tokens is not None:
            if max_tokens < 2:
                raise ValueError(f"max_tokens of {max_tokens}: [CLS] and [SEP] alone are two")
            ids = ids[:max_tokens - 2]
        return [self.cls_id] + ids + [self.sep_id]

    def pad(self, encoded: Sequence[Sequence[int]], npad: int) -> Tuple[np.ndarray, np.ndarray]:
        """id lists -> (ids int32 (n, npad) filled with ``[PAD]``, lengths int32 (n,))"""
        ids = np.full((len(encoded), npad), self.pad_id, np.int32)
        lens = np.empty(len(encoded), np.int32)
        for i, e in enumerate(encoded):
            if len(e) > npad:
                raise ValueError(f"text {i} has {len(e)} tokens, the rows hold {npad}")
            ids[i, :len(e)] = e
            lens[i] = len(e)
        return ids, lens
