"""Plain-torch restatement of the CLIP text tower + projection, parameterised by dtype (test infrastructure: the GPU tests compare
the HIP model against it, the CPU tests compare it against the transformers library in float64), plus the synthetic vocabulary,
the seeded weights and the texts both use.

Follows transformers/models/clip/modeling_clip.py: CLIPTextEmbeddings, CLIPTextTransformer (causal mask, CLIPEncoderLayer with
quick_gelu, final_layer_norm, the row of the first end-of-text id), CLIPTextModelWithProjection.text_projection.  Weights are
taken under the OpenAI key scheme, which is what marie_icr_amd.embeddings.load_clip_text_state stages.  Rows at positions past
the context length (the padding rows of a 77-token text in 80 rows) get a zero position row, as the library gives them; under
the causal mask they reach no earlier row.
"""
from __future__ import annotations

import gzip
import json
import os

import numpy as np
import torch

from marie_icr_amd.clip_tokenizer import EOT, GZ_NAME, SOT, bytes_to_unicode

# the merges of the synthetic vocabulary, in rank order: they build the</w>, invoice</w> and total</w>
MERGES = [("t", "h"), ("th", "e</w>"), ("i", "n"), ("in", "v"), ("o", "i"), ("c", "e</w>"), ("inv", "oi"), ("invoi", "ce</w>"),
          ("t", "o"), ("a", "l</w>"), ("to", "t"), ("tot", "al</w>")]
VOCAB_SIZE = 512 + len(MERGES) + 2

SMALL = dict(vocab=VOCAB_SIZE, dim=128, heads=2, ffn=512, depth=2, context=77, proj_dim=64)
VIT_B32_TEXT = dict(vocab=49408, dim=512, heads=8, ffn=2048, depth=12, context=77, proj_dim=512)

# sequence lengths 2, 3, 5, 5, 4, 9, 18, 11, 77
TEXTS = ["", "total", "the invoice total", "invoice total the", "the invoice", "Total: 12,50", "café naïve — ok",
         " ".join(["the"] * 9), " ".join(["invoice"] * 75)]
RANDOM_LENGTHS = (2, 7, 8, 9, 17, 33, 65, 77)


def make_vocab(directory: str) -> dict:
    """writes vocab.json + merges.txt (the ``transformers`` layout) and the .gz form of the synthetic vocabulary: 256 byte
    symbols, the same with </w>, MERGES, the two specials -> the paths"""
    symbols = list(bytes_to_unicode().values())
    vocab = symbols + [s + "</w>" for s in symbols] + ["".join(m) for m in MERGES] + [SOT, EOT]
    assert len(vocab) == VOCAB_SIZE == len(set(vocab))
    paths = {"vocab": os.path.join(directory, "vocab.json"), "merges": os.path.join(directory, "merges.txt"),
             "gz": os.path.join(directory, GZ_NAME)}
    with open(paths["vocab"], "w", encoding="utf-8") as f:
        json.dump({t: i for i, t in enumerate(vocab)}, f, ensure_ascii=False)
    lines = "".join(f"{a} {b}\n" for a, b in MERGES)
    with open(paths["merges"], "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + lines)
    with gzip.open(paths["gz"], "wb") as f:
        f.write(('"bpe_simple_vocab_16e6.txt#version: 0.2\n' + lines).encode("utf-8"))
    return paths


def make_state(cfg: dict, seed: int = 0) -> dict:
    """seeded OpenAI-scheme weights (float32 arrays): weights N(0, 0.05), token table N(0, 0.5), positions N(0, 0.1), LayerNorm
    gains 1 + 0.1 N, biases 0.02 N"""
    rng = np.random.default_rng(seed)
    D, F, E = cfg["dim"], cfg["ffn"], cfg["proj_dim"]

    def n(shape, s):
        return (rng.standard_normal(shape) * s).astype(np.float32)

    def ln(prefix, st):
        st[prefix + ".weight"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        st[prefix + ".bias"] = n((D,), 0.02)

    st = {"token_embedding.weight": n((cfg["vocab"], D), 0.5), "positional_embedding": n((cfg["context"], D), 0.1)}
    for i in range(cfg["depth"]):
        p = f"transformer.resblocks.{i}."
        ln(p + "ln_1", st)
        st[p + "attn.in_proj_weight"], st[p + "attn.in_proj_bias"] = n((3 * D, D), 0.05), n((3 * D,), 0.02)
        st[p + "attn.out_proj.weight"], st[p + "attn.out_proj.bias"] = n((D, D), 0.05), n((D,), 0.02)
        ln(p + "ln_2", st)
        st[p + "mlp.c_fc.weight"], st[p + "mlp.c_fc.bias"] = n((F, D), 0.05), n((F,), 0.02)
        st[p + "mlp.c_proj.weight"], st[p + "mlp.c_proj.bias"] = n((D, F), 0.05), n((D,), 0.02)
    ln("ln_final", st)
    st["text_projection"] = n((D, E), 0.05)
    return st


def to_transformers(st: dict) -> dict:
    """the same weights under the ``transformers`` key scheme (CLIPTextModelWithProjection.state_dict), torch tensors"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    D = st["token_embedding.weight"].shape[1]
    out = {"text_model.embeddings.token_embedding.weight": t(st["token_embedding.weight"]),
           "text_model.embeddings.position_embedding.weight": t(st["positional_embedding"]),
           "text_model.final_layer_norm.weight": t(st["ln_final.weight"]), "text_model.final_layer_norm.bias": t(st["ln_final.bias"]),
           "text_projection.weight": t(st["text_projection"].T)}
    names = {"attn.out_proj": "self_attn.out_proj", "ln_1": "layer_norm1", "ln_2": "layer_norm2", "mlp.c_fc": "mlp.fc1",
             "mlp.c_proj": "mlp.fc2"}
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in st:
        p, q = f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        for kind in ("weight", "bias"):
            w = st[p + "attn.in_proj_" + kind]
            for j, name in enumerate(("q_proj", "k_proj", "v_proj")):
                out[f"{q}self_attn.{name}.{kind}"] = t(w[j * D:(j + 1) * D])
            for a, b in names.items():
                out[f"{q}{b}.{kind}"] = t(st[f"{p}{a}.{kind}"])
        i += 1
    return out


def random_ids(cfg: dict, lengths=RANDOM_LENGTHS, seed: int = 5, pool: int = 2):
    """-> (ids int32 (n, npad), eot int32 (n,)): [SOT] + random ordinary ids + [EOT] of the given lengths, padded with id 0; the
    vocabulary's last two ids are the specials.  The sequences are prefixes of one random stream over `pool` random words (a
    repeated phrase): the long ones come out alike (cosine above 0.99 at ViT-B/32 text geometry), the short ones apart from
    them (below 0.7); independent streams over the whole vocabulary stay below 0.98."""
    rng = np.random.default_rng(seed)
    sot, eot_id = cfg["vocab"] - 2, cfg["vocab"] - 1
    words = rng.integers(0, cfg["vocab"] - 2, pool)
    stream = words[rng.integers(0, pool, max(lengths) - 2)]
    npad = (max(lengths) + 7) // 8 * 8
    ids, eot = np.zeros((len(lengths), npad), np.int32), np.zeros(len(lengths), np.int32)
    for i, n in enumerate(lengths):
        ids[i, :n] = [sot] + list(stream[:n - 2]) + [eot_id]
        eot[i] = n - 1
    return ids, eot


def _ln(x, st, prefix, eps=1e-5):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), st[prefix + ".weight"], st[prefix + ".bias"], eps)


def forward(state: dict, cfg: dict, ids, eot, dtype=torch.float64):
    """ids (n, T), eot (n,) -> (taps [depth + 1][n][T][D]: the residual stream after the embedding and after every layer,
    embeddings [n][E])"""
    st = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}
    D, H = cfg["dim"], cfg["heads"]
    ids = torch.from_numpy(np.asarray(ids)).long()
    n, T = ids.shape
    pos = torch.zeros((T, D), dtype=dtype)
    rows = min(T, st["positional_embedding"].shape[0])
    pos[:rows] = st["positional_embedding"][:rows]
    h = st["token_embedding.weight"][ids] + pos
    taps = [h]
    mask = torch.full((T, T), float("-inf"), dtype=dtype).triu(1)
    for i in range(cfg["depth"]):
        p = f"transformer.resblocks.{i}."
        y = _ln(h, st, p + "ln_1")
        qkv = y @ st[p + "attn.in_proj_weight"].T + st[p + "attn.in_proj_bias"]
        q, k, v = (t.reshape(n, T, H, D // H).transpose(1, 2) for t in qkv.split(D, dim=-1))
        a = torch.softmax(q @ k.transpose(-1, -2) * (D // H) ** -0.5 + mask, dim=-1) @ v
        h = h + a.transpose(1, 2).reshape(n, T, D) @ st[p + "attn.out_proj.weight"].T + st[p + "attn.out_proj.bias"]
        y = _ln(h, st, p + "ln_2") @ st[p + "mlp.c_fc.weight"].T + st[p + "mlp.c_fc.bias"]
        y = y * torch.sigmoid(1.702 * y)
        h = h + y @ st[p + "mlp.c_proj.weight"].T + st[p + "mlp.c_proj.bias"]
        taps.append(h)
    rows = h[torch.arange(n), torch.from_numpy(np.asarray(eot)).long()]
    emb = _ln(rows, st, "ln_final") @ st["text_projection"]
    return torch.stack(taps), emb


def causal_attention_fp64(q, k, v, heads: int) -> np.ndarray:
    """q, k, v (B, T, heads * 64), q in log2 units (scaled by head_dim^-0.5 * log2 e) -> softmax over keys 0 .. t, float64"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    B, T, D = q.shape
    split = lambda a: a.reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
    s = split(q) @ split(k).transpose(0, 1, 3, 2)
    s = np.where(np.tril(np.ones((T, T), bool)), s, -np.inf)
    p = np.exp2(s - s.max(-1, keepdims=True))
    out = (p / p.sum(-1, keepdims=True)) @ split(v)
    return out.transpose(0, 2, 1, 3).reshape(B, T, D)


def cosine_matrix(emb: torch.Tensor) -> torch.Tensor:
    x, y = emb[:, None, :], emb[None, :, :]
    return (x * y).sum(-1) / torch.clamp(x.norm(dim=-1) * y.norm(dim=-1), min=1e-8)
