"""CLIP's byte-pair tokeniser (host): ``clip.simple_tokenizer.SimpleTokenizer`` + ``clip.tokenize`` restated.

The text is cleaned (``html.unescape`` twice, strip, NFC, runs of white space to one space, strip, lower case), split by CLIP's
pattern, its UTF-8 bytes mapped through the GPT-2 byte/unicode table, and every piece merged by rank with ``</w>`` on its last
symbol.  A sequence is ``[SOT] + ids + [EOT]``.  ``ftfy`` is not applied (the package's own fallback when it is missing is what
``transformers.CLIPTokenizer`` does, and what this file matches).  A text longer than the context length raises ``ValueError``
unless ``truncation`` is set; ``clip.tokenize`` raises there too, and nothing here swallows it.

Vocabulary sources: ``vocab.json`` + ``merges.txt`` (the ``transformers`` layout) or OpenAI's ``bpe_simple_vocab_16e6.txt.gz``.
"""
from __future__ import annotations

import gzip
import html
import json
import os
import unicodedata
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import regex

SOT, EOT = "<|startoftext|>", "<|endoftext|>"
GZ_NAME = "bpe_simple_vocab_16e6.txt.gz"
_PATTERN = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"
_WHITE_SPACE = regex.compile(r"\s+")
_N_MERGES = 49152 - 256 - 2      # the slice both packages take of the merges file, after its header line


def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's table: every byte as a printable unicode character (the printable ones as themselves, the rest from 256 up)"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def _pairs(word: Tuple[str, ...]):
    return set(zip(word[:-1], word[1:]))


def clean(text: str) -> str:
    text = html.unescape(html.unescape(text)).strip()
    text = unicodedata.normalize("NFC", text)
    return _WHITE_SPACE.sub(" ", text).strip().lower()


class ClipTokenizer:
    def __init__(self, encoder: Dict[str, int], merges: Sequence[Tuple[str, str]], context_length: int = 77):
        self.encoder = dict(encoder)
        self.bpe_ranks = {tuple(m): i for i, m in enumerate(merges)}
        self.byte_encoder = bytes_to_unicode()
        for special in (SOT, EOT):
            if special not in self.encoder:
                raise ValueError(f"CLIP vocabulary has no {special}")
        self.sot, self.eot = self.encoder[SOT], self.encoder[EOT]
        self.cache = {SOT: SOT, EOT: EOT}
        self.id_cache: Dict[str, List[int]] = {}      # a piece of the split pattern -> its ids
        self.pat = regex.compile(_PATTERN, regex.IGNORECASE)
        self.context_length = int(context_length)

    # -- vocabulary sources ----------------------------------------------------------------------------------------------
    @staticmethod
    def _read_merges(lines: List[str]) -> List[Tuple[str, str]]:
        return [tuple(line.split()) for line in lines[1:_N_MERGES + 1] if line.strip()]

    @classmethod
    def from_files(cls, vocab_json: str, merges_txt: str, context_length: int = 77) -> "ClipTokenizer":
        """the ``transformers`` layout"""
        with open(vocab_json, encoding="utf-8") as f:
            encoder = json.load(f)
        with open(merges_txt, encoding="utf-8") as f:
            merges = cls._read_merges(f.read().strip().split("\n"))
        return cls(encoder, merges, context_length)

    @classmethod
    def from_gz(cls, path: str, context_length: int = 77) -> "ClipTokenizer":
        """OpenAI's ``bpe_simple_vocab_16e6.txt.gz``: the vocabulary is the 256 byte symbols, the same with ``</w>``, the
        merges, then the two specials"""
        merges = cls._read_merges(gzip.open(path).read().decode("utf-8").split("\n"))
        vocab = list(bytes_to_unicode().values())
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + [SOT, EOT]
        return cls(dict(zip(vocab, range(len(vocab)))), merges, context_length)

    @classmethod
    def from_dir(cls, model_dir, context_length: int = 77) -> Optional["ClipTokenizer"]:
        """the vocabulary a model directory holds, or None"""
        if model_dir is None or not os.path.isdir(model_dir):
            return None
        vocab, merges, gz = (os.path.join(model_dir, n) for n in ("vocab.json", "merges.txt", GZ_NAME))
        if os.path.isfile(vocab) and os.path.isfile(merges):
            return cls.from_files(vocab, merges, context_length)
        if os.path.isfile(gz):
            return cls.from_gz(gz, context_length)
        return None

    # -- encoding --------------------------------------------------------------------------------------------------------
    def bpe(self, token: str) -> str:
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        pairs = _pairs(word)
        if not pairs:
            return token + "</w>"
        while True:
            bigram = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            merged, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == first and word[i + 1] == second:
                    merged.append(first + second)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = tuple(merged)
            if len(word) == 1:
                break
            pairs = _pairs(word)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def encode(self, text: str) -> List[int]:
        """the ids of ``text`` without the specials"""
        ids: List[int] = []
        for piece in self.pat.findall(clean(text)):
            piece_ids = self.id_cache.get(piece)
            if piece_ids is None:
                token = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
                piece_ids = self.id_cache[piece] = [self.encoder[t] for t in self.bpe(token).split(" ")]
            ids.extend(piece_ids)
        return ids

    def tokenize(self, text: str, truncation: bool = False, context_length: Optional[int] = None) -> List[int]:
        """``[SOT] + ids + [EOT]``, at most the context length"""
        limit = int(context_length or self.context_length)
        ids = [self.sot] + self.encode(text) + [self.eot]
        if len(ids) > limit:
            if not truncation:
                raise ValueError(f"text of {len(ids)} tokens is too long for the context length of {limit}: {text[:60]!r}")
            ids = ids[:limit]
            ids[-1] = self.eot
        return ids

    def encode_batch(self, texts: Sequence[str], truncation: bool = False,
                     context_length: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """-> (ids int32 (n, npad), eot int32 (n,)): npad is the longest sequence of the call rounded up to a multiple of 8,
        the padding id is 0, eot[i] the index of the EOT appended to text i"""
        seqs = [self.tokenize(t, truncation, context_length) for t in texts]
        npad = (max((len(s) for s in seqs), default=2) + 7) // 8 * 8
        ids = np.zeros((len(seqs), npad), np.int32)
        eot = np.zeros(len(seqs), np.int32)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = s
            eot[i] = len(s) - 1
        return ids, eot
