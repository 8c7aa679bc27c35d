"""Float64 restatement of LongformerForSequenceClassification as pipeline("text-classification") runs it (global attention on <s>
alone), written as a per-token set definition — no chunks, no padding to the window — and the seeded tiny models, texts and toy
tokenizer files of tests/golden/longformer.npz (written by tests/make_longformer_golden.py from the transformers library).

A text has n tokens <s> ... </s>.  In layer l, with the one-sided window w = attention_window[l] / 2:
  * query i >= 1 attends to {0} U {j : max(1, i - w) <= j <= min(n - 1, i + w)} with the local q, k, v; key 0 counts once;
  * query 0 attends to every j < n with query_global / key_global / value_global;
then attention.output.dense + residual + LayerNorm and the erf-GELU MLP as in BERT; logits = out_proj(tanh(dense(h_0))).

With f16=True every value the f16 build holds in float16 is rounded to it (the GEMM operands, q | k | v, k_g | v_g, the
probabilities of the windowed kernel as the second product's operand, the attention output); the stream, the global query, the
soft-max state and the head stay unrounded, as fp32 in the kernels.
"""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402
import sentence_families_ref as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "longformer.npz")
LOG2E = 1.4426950408889634

VOCAB = 5 + 256 + len(S.BPE_MERGES)      # sentence_families_ref.bpe_vocab()
MODEL_MAX_LENGTH = 192                   # tokenizer_config.json: what truncation=True cuts to
# A: a window per layer, three labels (soft-max).  B: one window for all layers, one label (sigmoid)
MODELS = {
    "A": dict(vocab=VOCAB, max_position=MODEL_MAX_LENGTH + 2, type_vocab=1, dim=128, heads=2, depth=2, ffn=256, eps=1e-5,
              position="absolute", mlp="gelu", attention_window=[16, 48], num_labels=3, logit_gain=6.0),
    "B": dict(vocab=VOCAB, max_position=MODEL_MAX_LENGTH + 2, type_vocab=1, dim=128, heads=2, depth=2, ffn=256, eps=1e-5,
              position="absolute", mlp="gelu", attention_window=32, num_labels=1, logit_gain=6.0),
}
SEEDS = {"A": 31, "B": 32}
ROWS_PER_TEXT = 4      # stored rows of every tap: the first two and the last two tokens

# token counts of the golden's texts, <s> and </s> included: the shortest text, one-sided windows 8 and 24 met and passed, the
# 64-query block edge, past 2 * 24 + 2 + 64 = 114, and one text that truncation cuts to MODEL_MAX_LENGTH
TEXT_TOKENS = [2, 3, 9, 10, 17, 25, 26, 50, 64, 65, 120, 161, 230]
_WORDS = ["the", "invoice", "total", "amount", "due", "12", "50", "pay", "no", "resume", "to", "in", "1250", "don't", "co.", "a"]


def windows(cfg):
    """the one-sided window of every layer"""
    aw = cfg["attention_window"]
    aw = [aw] * cfg["depth"] if isinstance(aw, int) else list(aw)
    assert len(aw) == cfg["depth"] and all(a > 0 and a % 2 == 0 for a in aw)
    return [a // 2 for a in aw]


def head_function(cfg):
    return "sigmoid" if cfg["num_labels"] == 1 else "softmax"


def id2label(cfg):
    return {i: f"LABEL_{i}" for i in range(cfg["num_labels"])}


def config_json(cfg):
    """the config.json LongformerForSequenceClassification.save_pretrained writes for `cfg` (the fields the loader reads)"""
    return dict(model_type="longformer", architectures=["LongformerForSequenceClassification"], vocab_size=cfg["vocab"],
                hidden_size=cfg["dim"], num_attention_heads=cfg["heads"], num_hidden_layers=cfg["depth"], intermediate_size=cfg["ffn"],
                max_position_embeddings=cfg["max_position"], type_vocab_size=cfg["type_vocab"], layer_norm_eps=cfg["eps"],
                hidden_act="gelu", pad_token_id=1, bos_token_id=0, eos_token_id=2, sep_token_id=2,
                attention_window=cfg["attention_window"] if isinstance(cfg["attention_window"], int) else list(cfg["attention_window"]),
                id2label={str(i): v for i, v in id2label(cfg).items()}, label2id={v: i for i, v in id2label(cfg).items()})


def make_state(cfg, seed):
    """seeded O(1) weights under LongformerForSequenceClassification's keys: bert_text_ref.make_state's recipe for the encoder, the
    global projections drawn like the local ones, and a head whose out_proj carries `logit_gain`, so that the labels differ from
    text to text.  Every tensor on bert_text_ref.quantize_state's grid: exact in float16, float32 and float64"""
    rng = np.random.default_rng(seed + 700)
    D, L = cfg["dim"], cfg["num_labels"]
    sd = R.make_state(cfg, seed)
    for n in range(cfg["depth"]):
        p = f"encoder.layer.{n}.attention.self."
        for name in ("query", "key", "value"):
            sd[p + f"{name}_global.weight"] = (rng.standard_normal((D, D)) / math.sqrt(D) * (2.0 if name != "value" else 1.0)).astype(np.float32)
            sd[p + f"{name}_global.bias"] = (0.2 * rng.standard_normal(D)).astype(np.float32)
    out = {"longformer." + k: v for k, v in sd.items()}
    out["classifier.dense.weight"] = (rng.standard_normal((D, D)) / math.sqrt(D)).astype(np.float32)
    out["classifier.dense.bias"] = (0.2 * rng.standard_normal(D)).astype(np.float32)
    out["classifier.out_proj.weight"] = (cfg["logit_gain"] * rng.standard_normal((L, D)) / math.sqrt(D)).astype(np.float32)
    out["classifier.out_proj.bias"] = (0.2 * rng.standard_normal(L)).astype(np.float32)
    return R.quantize_state(out)[0]


# ---------------------------------------------------------------------------------------------------- the kernels' definitions
def window_attention(q, k, v, lens, heads, w, f16=False):
    """q, k, v float64 (B, npad, heads * hd), q in log2 units.  Query i of text b: soft-max over key 0 and the keys
    max(1, i - w) .. min(lens[b] - 1, i + w).  Row 0 and the rows >= lens[b] are not part of the definition (zeros here).
    f16: the probabilities are rounded to float16 as the operand of the second product, their sum is not"""
    B, npad, D = q.shape
    hd = D // heads
    out = np.zeros_like(q)
    for b in range(B):
        n = int(lens[b])
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        seen = (j == 0) | ((j >= 1) & (np.abs(i - j) <= w))
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            s = np.where(seen, q[b, :n, c] @ k[b, :n, c].T, -np.inf)
            p = np.exp2(s - s.max(-1, keepdims=True))
            out[b, :n, c] = ((R.r16(p) if f16 else p) @ v[b, :n, c]) / p.sum(-1, keepdims=True)
        out[b, 0] = 0.0
    return out


def global_row(qg, kg, vg, lens, heads):
    """qg (B, D) in log2 units, kg, vg (B, npad, D) -> (B, D): query 0's soft-max over the lens[b] keys, per head"""
    B, D = qg.shape
    hd = D // heads
    out = np.zeros_like(qg)
    for b in range(B):
        n = int(lens[b])
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            s = kg[b, :n, c] @ qg[b, c]
            p = np.exp2(s - s.max())
            out[b, c] = (p @ vg[b, :n, c]) / p.sum()
    return out


def scores_of(logits, function):
    """the pipeline's post-processing: 'softmax', 'sigmoid' or 'none'"""
    z = np.asarray(logits, np.float64)
    if function == "softmax":
        e = np.exp(z - z.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)
    if function == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    return z


def cls_head(h0, dense_w, dense_b, out_w, out_b, function):
    """h0 (B, D) -> (logits, scores) (B, L)"""
    y = np.tanh(np.asarray(h0, np.float64) @ np.asarray(dense_w, np.float64).T + dense_b)
    logits = y @ np.asarray(out_w, np.float64).T + out_b
    return logits, scores_of(logits, function)


def forward(sd, cfg, ids, lens, f16=False):
    """-> (taps float64 (depth + 1, B, npad, D): the stream after the embedding LayerNorm and after every layer — rows >= lens[b]
    mean nothing —, logits (B, L))"""
    rnd = R.r16 if f16 else (lambda x: np.asarray(x, np.float64))
    W = {(k[11:] if k.startswith("longformer.") else k): np.asarray(v, np.float64) for k, v in sd.items()}
    D, heads, eps = cfg["dim"], cfg["heads"], cfg["eps"]
    scale = LOG2E / math.sqrt(D // heads)
    ids = np.asarray(ids)
    B, npad = ids.shape
    x = W["embeddings.word_embeddings.weight"][ids] + W["embeddings.token_type_embeddings.weight"][0]
    x = x + W["embeddings.position_embeddings.weight"][2:2 + npad]
    h = R.layer_norm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps)
    taps = [h]
    for n, w in enumerate(windows(cfg)):
        p = f"encoder.layer.{n}."
        a = p + "attention.self."
        ht = rnd(h)
        q = rnd(ht @ rnd(W[a + "query.weight"] * scale).T + W[a + "query.bias"] * scale)
        k = rnd(ht @ rnd(W[a + "key.weight"]).T + W[a + "key.bias"])
        v = rnd(ht @ rnd(W[a + "value.weight"]).T)       # the value bias is added behind the soft-max
        ao = window_attention(q, k, v, lens, heads, w, f16)
        qg = ht[:, 0] @ rnd(W[a + "query_global.weight"] * scale).T + W[a + "query_global.bias"] * scale
        kg = rnd(ht @ rnd(W[a + "key_global.weight"]).T + W[a + "key_global.bias"])
        vg = rnd(ht @ rnd(W[a + "value_global.weight"]).T)
        # row 0: the output projection's folded bias adds W_o b_v to every row
        ao[:, 0] = global_row(qg, kg, vg, lens, heads) + (W[a + "value_global.bias"] - W[a + "value.bias"])
        ao = rnd(ao)
        wo = W[p + "attention.output.dense.weight"]
        y = ao @ rnd(wo).T + (W[p + "attention.output.dense.bias"] + wo @ W[a + "value.bias"]) + h
        h = R.layer_norm(y, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        ht = rnd(h)
        hid = rnd(R.gelu(ht @ rnd(W[p + "intermediate.dense.weight"]).T + W[p + "intermediate.dense.bias"]))
        y = hid @ rnd(W[p + "output.dense.weight"]).T + W[p + "output.dense.bias"] + h
        h = R.layer_norm(y, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
        taps.append(h)
    logits, _ = cls_head(h[:, 0], W["classifier.dense.weight"], W["classifier.dense.bias"], W["classifier.out_proj.weight"],
                         W["classifier.out_proj.bias"], "none")
    return np.stack(taps), logits


# ---------------------------------------------------------------------------------------------------- texts and files
def make_texts(count_tokens, seed=5):
    """one text per entry of TEXT_TOKENS: words of _WORDS joined by blanks until the text has that many tokens (<s>, </s>
    included) as `count_tokens(text)` counts them without truncation; the 2-token text is empty"""
    rng = np.random.default_rng(seed)
    texts = []
    for target in TEXT_TOKENS:
        words = []
        while count_tokens(" ".join(words)) < target:
            words.append(_WORDS[int(rng.integers(len(_WORDS)))])
        while count_tokens(" ".join(words)) != target:      # a word of several tokens overshot: trade it for one-token words
            if count_tokens(" ".join(words)) > target:
                words.pop()
            else:
                words.append("a")
        texts.append(" ".join(words))
    return texts


def stored_rows(lens):
    """the ROWS_PER_TEXT rows of every text the golden stores of each tap (a 2- or 3-token text repeats some)"""
    return np.array([[0, min(1, n - 1), max(n - 2, 0), n - 1] for n in lens], np.int32)


def write_model_dir(directory, name, state=None):
    """a model directory as save_pretrained + the tokenizer's save leave it: config.json, pytorch_model.bin, vocab.json, merges.txt,
    tokenizer_config.json"""
    import torch

    cfg = MODELS[name]
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "config.json"), "w", encoding="utf-8") as f:
        json.dump(config_json(cfg), f)
    with open(os.path.join(directory, "tokenizer_config.json"), "w", encoding="utf-8") as f:
        json.dump(dict(model_max_length=MODEL_MAX_LENGTH, tokenizer_class="LongformerTokenizer"), f)
    S.write_bpe_files(directory)
    sd = state if state is not None else make_state(cfg, SEEDS[name])
    torch.save({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()}, os.path.join(directory, "pytorch_model.bin"))
    return directory


def load_golden(path=GOLDEN):
    """-> {"A" / "B": dict(cfg, state, ids [list of int32 arrays], lens, rows, tap_rows (depth + 1, n, ROWS_PER_TEXT, D), logits,
    scores)}, texts.  The weights are not stored: make_state regenerates them from the seed"""
    z = np.load(path)
    texts = json.loads(str(z["texts"]))
    lens = z["lens"].astype(np.int32)
    flat = z["ids"].astype(np.int32)
    at = np.concatenate([[0], np.cumsum(lens)])
    ids = [flat[at[i]:at[i + 1]] for i in range(len(lens))]
    models = {}
    for name, cfg in MODELS.items():
        models[name] = dict(cfg=cfg, state=make_state(cfg, SEEDS[name]), ids=ids, lens=lens, rows=stored_rows(lens),
                            tap_rows=z[f"{name}/tap_rows"], logits=z[f"{name}/logits"], scores=z[f"{name}/scores"])
    return models, texts


def pad_ids(ids, npad, pad_id=1):
    out = np.full((len(ids), npad), pad_id, np.int32)
    for i, e in enumerate(ids):
        out[i, :len(e)] = e
    return out
