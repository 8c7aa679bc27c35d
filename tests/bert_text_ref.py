"""float64 restatement of the BERT sentence encoders (marie_icr_amd/csrc/berttext_api.hip): Hugging Face BERT and the JinaBERT
variant (ALiBi, GEGLU), mean and [CLS] pooling, optional L2 normalisation.  tests/test_berttext_cpu.py pins its plain-BERT path to
transformers.BertModel through tests/golden/bert_text.npz; ALiBi and GEGLU are restated from the descriptions in DESIGN.md.

`forward(..., f16=True)` rounds to float16 where the f16 mode of the encoder does — the GEMM weights (the score scale folded into
W_q first), every GEMM input and every GEMM output that is kept in f16 (q | k, V^T, the attention output, the MLP hidden rows), and
the probabilities as the operand of the second attention product — and keeps float64 everywhere else, so that
max |f16 restatement - float64 restatement| measures what those roundings cost.
"""
import math

import numpy as np

LOG2E = 1.4426950408889634

# config A / B of tests/make_bert_text_golden.py, and B as JinaBERT
CONFIG_A = dict(vocab=80, max_position=128, type_vocab=2, dim=64, heads=2, depth=2, ffn=256, eps=1e-12, position="absolute", mlp="gelu")
CONFIG_B = dict(CONFIG_A, dim=128)
CONFIG_B_JINA = dict(CONFIG_B, position="alibi", mlp="geglu")


def config_json(cfg):
    """the config.json a checkpoint of `cfg` carries"""
    out = dict(vocab_size=cfg["vocab"], hidden_size=cfg["dim"], num_attention_heads=cfg["heads"], num_hidden_layers=cfg["depth"],
               intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_position"], type_vocab_size=cfg["type_vocab"],
               layer_norm_eps=cfg["eps"], hidden_act="gelu", position_embedding_type=cfg["position"])
    if cfg["mlp"] == "geglu":
        out["feed_forward_type"] = "geglu"
    return out


def alibi_slopes(n):
    """2^(-8 (i + 1) / n) for n a power of two; otherwise the slopes of the largest power of two p <= n, then every other slope
    of 2 p from its first"""
    def pow2(p):
        return [2.0 ** (-8.0 * (i + 1) / p) for i in range(p)]
    p = 2 ** int(math.floor(math.log2(n)))
    return np.array(pow2(p) + pow2(2 * p)[0::2][:n - p])


def make_state(cfg, seed=0):
    """seeded weights of `cfg` under the checkpoint's keys: matrices of std fan_in^-0.5, random LayerNorm gains and biases, random
    biases (the default std-0.02 initialisation hides errors)"""
    rng = np.random.default_rng(seed)
    D, F = cfg["dim"], cfg["ffn"]

    def mat(o, i):
        return (rng.standard_normal((o, i)) / math.sqrt(i)).astype(np.float32)

    def vec(n, scale=0.2):
        return (scale * rng.standard_normal(n)).astype(np.float32)

    def ln(prefix, sd):
        sd[prefix + ".weight"] = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
        sd[prefix + ".bias"] = vec(D)

    sd = {"embeddings.word_embeddings.weight": rng.standard_normal((cfg["vocab"], D)).astype(np.float32),
          "embeddings.token_type_embeddings.weight": (0.5 * rng.standard_normal((cfg["type_vocab"], D))).astype(np.float32)}
    if cfg["position"] == "absolute":
        sd["embeddings.position_embeddings.weight"] = (0.5 * rng.standard_normal((cfg["max_position"], D))).astype(np.float32)
    ln("embeddings.LayerNorm", sd)
    for n in range(cfg["depth"]):
        p = f"encoder.layer.{n}."
        for name in ("query", "key", "value"):
            sd[p + f"attention.self.{name}.weight"] = mat(D, D) * (2.0 if name != "value" else 1.0)      # scores of a few units
            sd[p + f"attention.self.{name}.bias"] = vec(D)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = mat(D, D), vec(D)
        ln(p + "attention.output.LayerNorm", sd)
        if cfg["mlp"] == "geglu":
            sd[p + "mlp.gated_layers.weight"] = mat(2 * F, D)
            sd[p + "mlp.wo.weight"], sd[p + "mlp.wo.bias"] = mat(D, F), vec(D)
            ln(p + "mlp.layernorm", sd)
        else:
            sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"] = mat(F, D), vec(F)
            sd[p + "output.dense.weight"], sd[p + "output.dense.bias"] = mat(D, F), vec(D)
            ln(p + "output.LayerNorm", sd)
    return sd


def make_ids(cfg, lens, npad, seed=0, cls_id=2, sep_id=3, pad_id=0):
    """[CLS] random ids [SEP] [PAD] ... of the given lengths -> ids int32 (n, npad)"""
    rng = np.random.default_rng(seed + 1000)
    ids = np.full((len(lens), npad), pad_id, np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(5, cfg["vocab"], n)
        ids[i, 0] = cls_id
        if n > 1:
            ids[i, n - 1] = sep_id
    return ids


def r16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def gelu(x):
    erf = np.vectorize(math.erf, otypes=[np.float64])
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def attention(q, k, v, lens, heads, slopes=None, f16=False):
    """q, k, v float64 (B, npad, heads * hd), q in log2 units (scaled by hd^-0.5 * log2(e)); text b attends to its first lens[b]
    keys; slopes (heads,) in the same log2 units or None.  f16: the probabilities are rounded to float16 as the operand of the
    second product, their sum is not"""
    B, npad, D = q.shape
    hd = D // heads
    out = np.zeros_like(q)
    pos = np.arange(npad)
    dist = np.abs(pos[:, None] - pos[None, :]).astype(np.float64)
    for b in range(B):
        n = int(lens[b])
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            s = q[b, :, c] @ k[b, :n, c].T
            if slopes is not None:
                s = s - slopes[h] * dist[:, :n]
            p = np.exp2(s - s.max(-1, keepdims=True))
            out[b, :, c] = ((r16(p) if f16 else p) @ v[b, :n, c]) / p.sum(-1, keepdims=True)
    return out


def pool(h, lens, mode="mean", normalize=False):
    if mode == "cls":
        emb = h[:, 0].copy()
    else:
        emb = np.stack([h[b, :int(n)].sum(0) / max(float(n), 1e-9) for b, n in enumerate(lens)])
    if normalize:
        emb = emb / np.maximum(np.sqrt((emb ** 2).sum(-1, keepdims=True)), 1e-12)
    return emb


def forward(sd, cfg, ids, lens, mode="mean", normalize=False, f16=False):
    """-> (taps float64 (depth + 1, B, npad, D): the stream after the embedding LayerNorm and after every layer, embeddings
    (B, D)).  Rows >= lens[b] are computed as the encoder computes them: queries like any other, never keys."""
    rnd = r16 if f16 else (lambda x: np.asarray(x, np.float64))
    W = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    D, heads, F, eps = cfg["dim"], cfg["heads"], cfg["ffn"], cfg["eps"]
    scale = LOG2E / math.sqrt(D // heads)
    ids = np.asarray(ids)
    B, npad = ids.shape
    x = W["embeddings.word_embeddings.weight"][ids] + W["embeddings.token_type_embeddings.weight"][0]
    if cfg["position"] == "absolute":
        x = x + W["embeddings.position_embeddings.weight"][:npad]
    h = layer_norm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps)
    slopes = alibi_slopes(heads) * LOG2E if cfg["position"] == "alibi" else None
    taps = [h]
    for n in range(cfg["depth"]):
        p = f"encoder.layer.{n}."
        ht = rnd(h)
        q = rnd(ht @ rnd(W[p + "attention.self.query.weight"] * scale).T + W[p + "attention.self.query.bias"] * scale)
        k = rnd(ht @ rnd(W[p + "attention.self.key.weight"]).T + W[p + "attention.self.key.bias"])
        v = rnd(ht @ rnd(W[p + "attention.self.value.weight"]).T)       # the value bias is added behind the soft-max
        ao = rnd(attention(q, k, v, lens, heads, slopes, f16))
        wo = W[p + "attention.output.dense.weight"]
        y = ao @ rnd(wo).T + (W[p + "attention.output.dense.bias"] + wo @ W[p + "attention.self.value.bias"]) + h
        h = layer_norm(y, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        ht = rnd(h)
        if cfg["mlp"] == "geglu":
            u = rnd(ht @ rnd(W[p + "mlp.gated_layers.weight"]).T)
            hid = rnd(gelu(u[..., :F]) * u[..., F:])
            y = hid @ rnd(W[p + "mlp.wo.weight"]).T + W[p + "mlp.wo.bias"] + h
            h = layer_norm(y, W[p + "mlp.layernorm.weight"], W[p + "mlp.layernorm.bias"], eps)
        else:
            hid = rnd(gelu(ht @ rnd(W[p + "intermediate.dense.weight"]).T + W[p + "intermediate.dense.bias"]))
            y = hid @ rnd(W[p + "output.dense.weight"]).T + W[p + "output.dense.bias"] + h
            h = layer_norm(y, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
        taps.append(h)
    return np.stack(taps), pool(h, lens, mode, normalize)


def cosine_matrix(emb):
    emb = np.asarray(emb, np.float64)
    n = np.sqrt((emb ** 2).sum(-1))
    return (emb @ emb.T) / np.maximum(n[:, None] * n[None, :], 1e-8)


def valid_rows(lens, npad):
    """bool (B, npad): the rows somebody reads"""
    return np.arange(npad)[None, :] < np.asarray(lens)[:, None]


# ---------------------------------------------------------------------------------------------------- tests/golden/bert_text.npz
def quantize_state(sd):
    """every tensor on a grid of 255 steps of a power of two (int8 x 2^e): exact in float16, float32 and float64 alike, and a
    quarter of the bytes in the golden file -> (the tensors on the grid as float32, {key: (int8 array, e)})"""
    out, packed = {}, {}
    for key, w in sd.items():
        e = int(math.ceil(math.log2(float(np.abs(w).max()) / 127.0)))
        q = np.clip(np.rint(np.asarray(w, np.float64) / 2.0 ** e), -127, 127).astype(np.int8)
        out[key] = (q.astype(np.float64) * 2.0 ** e).astype(np.float32)
        packed[key] = (q, e)
    return out, packed


def load_golden(path):
    """-> ({"A" / "B": dict(state, ids, lens, hidden (depth + 1, B, npad, D), mean, mean_norm, cls)}, dict(vocab, do_lower_case,
    texts, tokens, ids) of the tokenizer cases)"""
    import json

    z = np.load(path)
    models = {}
    for name in ("A", "B"):
        keys = json.loads(str(z[f"{name}/keys"]))
        exps = z[f"{name}/exps"]
        state = {k: (z[f"{name}/w{i}"].astype(np.float64) * 2.0 ** int(exps[i])).astype(np.float32) for i, k in enumerate(keys)}
        models[name] = dict(state=state, **{k: z[f"{name}/{k}"] for k in ("ids", "lens", "hidden", "mean", "mean_norm", "cls")})
    return models, json.loads(str(z["tokenizer"]))
