"""float64 restatement of the three sentence-encoder families beside BERT that marie_icr_amd/csrc/berttext_api.hip runs — MPNet
(position rows from pad_id + 1, no token types, a relative attention bias shared by the layers), RoBERTa (position rows from
pad_id + 1, one token type) and DistilBERT (no token types, its own key names) — and what tests/make_sentence_families_golden.py,
tests/test_sentence_families_cpu.py and tests/test_sentence_families_gpu.py share: the models of
tests/golden/sentence_families.npz, its loader and the toy vocabularies.  tests/test_sentence_families_cpu.py pins `forward` to
transformers' MPNetModel, RobertaModel and DistilBertModel through that golden.

The checkpoints here carry each family's own key names; `canonical` maps them onto the BERT names bert_text_ref.py uses, written
out on its own and not taken from the loader under test.  MPNet's bucket of a relative position is not restated: the golden
stores what MPNetEncoder.relative_position_bucket returns for -600 .. 600 (`buckets`), and `rel_table` gathers from it.

`forward(..., f16=True)` rounds where the f16 mode of the encoder does, as bert_text_ref.forward; the bias table stays unrounded
(it is fp32 in both modes).
"""
import json
import math
import os

import numpy as np

import bert_text_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sentence_families.npz")
LOG2E = R.LOG2E
LENS, NPAD = [3, 16, 17, 24], 24
LONG_LENS, LONG_NPAD = [129, 131, 257], 264
BUCKET_SPAN = 600          # the golden's buckets cover relative positions -600 .. 600
REL_BUCKETS, REL_MAX_DISTANCE = 32, 128

# family, geometry; pad_id is the id HF counts positions around (MPNet, RoBERTa: position row pad_id + 1 + t)
MODELS = {
    "mpnet_a": dict(family="mpnet", vocab=80, max_position=136, type_vocab=0, dim=64, heads=2, depth=2, ffn=128, eps=1e-5, pos_offset=2),
    "mpnet_b": dict(family="mpnet", vocab=80, max_position=520, type_vocab=0, dim=128, heads=2, depth=2, ffn=128, eps=1e-5, pos_offset=2),
    "roberta": dict(family="roberta", vocab=320, max_position=136, type_vocab=1, dim=128, heads=2, depth=2, ffn=128, eps=1e-5, pos_offset=2),
    "distilbert": dict(family="distilbert", vocab=80, max_position=128, type_vocab=0, dim=64, heads=2, depth=2, ffn=128, eps=1e-12, pos_offset=0),
}
SEEDS = {"mpnet_a": 21, "mpnet_b": 22, "roberta": 23, "distilbert": 24}
# ids of the special tokens in the toy vocabularies below
SPECIAL_IDS = {"mpnet": dict(cls_id=0, pad_id=1, sep_id=2), "roberta": dict(cls_id=0, pad_id=1, sep_id=2),
               "distilbert": dict(cls_id=2, pad_id=0, sep_id=3)}

_MPNET = {"attention.self.query": "attention.attn.q", "attention.self.key": "attention.attn.k", "attention.self.value": "attention.attn.v",
          "attention.output.dense": "attention.attn.o", "attention.output.LayerNorm": "attention.LayerNorm",
          "intermediate.dense": "intermediate.dense", "output.dense": "output.dense", "output.LayerNorm": "output.LayerNorm"}
_DISTIL = {"attention.self.query": "attention.q_lin", "attention.self.key": "attention.k_lin", "attention.self.value": "attention.v_lin",
           "attention.output.dense": "attention.out_lin", "attention.output.LayerNorm": "sa_layer_norm",
           "intermediate.dense": "ffn.lin1", "output.dense": "ffn.lin2", "output.LayerNorm": "output_layer_norm"}


def own_key(family, key):
    """the family's name of the canonical (BERT) key"""
    if family == "roberta" or not key.startswith("encoder.layer."):
        return key
    _, _, n, rest = key.split(".", 3)
    module, leaf = rest.rsplit(".", 1)
    if family == "mpnet":
        return f"encoder.layer.{n}.{_MPNET[module]}.{leaf}"
    return f"transformer.layer.{n}.{_DISTIL[module]}.{leaf}"


def canonical(sd, family):
    """a checkpoint under the family's names -> under BERT's (the relative attention bias keeps its name)"""
    back = {}
    for key in sd:
        parts = key.split(".")
        if family == "mpnet" and key.startswith("encoder.layer."):
            module = ".".join(parts[3:-1])
            name = {v: k for k, v in _MPNET.items()}[module]
            back[key] = f"encoder.layer.{parts[2]}.{name}.{parts[-1]}"
        elif family == "distilbert" and key.startswith("transformer.layer."):
            module = ".".join(parts[3:-1])
            name = {v: k for k, v in _DISTIL.items()}[module]
            back[key] = f"encoder.layer.{parts[2]}.{name}.{parts[-1]}"
        else:
            back[key] = key
    return {back[k]: v for k, v in sd.items()}


def config_json(cfg):
    """the config.json a checkpoint of `cfg` carries, with the names its family uses"""
    if cfg["family"] == "distilbert":
        return dict(model_type="distilbert", vocab_size=cfg["vocab"], dim=cfg["dim"], n_heads=cfg["heads"], n_layers=cfg["depth"],
                    hidden_dim=cfg["ffn"], max_position_embeddings=cfg["max_position"], activation="gelu", sinusoidal_pos_embds=False,
                    pad_token_id=0)
    out = dict(model_type=cfg["family"], vocab_size=cfg["vocab"], hidden_size=cfg["dim"], num_attention_heads=cfg["heads"],
               num_hidden_layers=cfg["depth"], intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_position"],
               layer_norm_eps=cfg["eps"], hidden_act="gelu", pad_token_id=1)
    if cfg["family"] == "mpnet":
        out["relative_attention_num_buckets"] = REL_BUCKETS
    else:
        out["type_vocab_size"] = cfg["type_vocab"]
    return out


def make_state(cfg, seed):
    """seeded O(1) weights of `cfg` under its family's key names (bert_text_ref.make_state's recipe, then renamed), MPNet's bias
    table of a few units on top"""
    bert = dict(cfg, type_vocab=max(cfg["type_vocab"], 1), position="absolute", mlp="gelu")
    sd = R.make_state(bert, seed)
    if not cfg["type_vocab"]:
        del sd["embeddings.token_type_embeddings.weight"]
    out = {own_key(cfg["family"], k): v for k, v in sd.items()}
    if cfg["family"] == "mpnet":
        rng = np.random.default_rng(seed + 500)
        out["encoder.relative_attention_bias.weight"] = (1.5 * rng.standard_normal((REL_BUCKETS, cfg["heads"]))).astype(np.float32)
    return out


def make_ids(cfg, lens, npad, seed):
    return R.make_ids(cfg, lens, npad, seed, **SPECIAL_IDS[cfg["family"]])


def rel_table(weight, buckets, radius=REL_MAX_DISTANCE):
    """weight (n_buckets, heads), buckets: the golden's bucket of every relative position key - query in -BUCKET_SPAN ..
    BUCKET_SPAN -> (heads, 2 radius + 1) over d = query - key, the bias of (query i, key j) at [h, clamp(i - j) + radius].  The
    clamp is exact only where the bucket is constant past the radius: asserted over the golden's span"""
    buckets = np.asarray(buckets)
    at = lambda rel: buckets[rel + BUCKET_SPAN]      # noqa: E731
    assert (at(np.arange(radius, BUCKET_SPAN + 1)) == at(radius)).all() and (at(np.arange(-BUCKET_SPAN, -radius + 1)) == at(-radius)).all()
    d = np.arange(-radius, radius + 1)
    return np.asarray(weight, np.float64)[at(-d)].T.copy()


def attention(q, k, v, lens, heads, table=None, f16=False):
    """bert_text_ref.attention with a relative-distance table in place of the slopes: q, k, v float64 (B, npad, heads * hd), q in
    log2 units; table (heads, 2 R + 1) in the same units or None, the score of (query i, key j) gets table[h, clamp(i - j, -R, R) + R]"""
    B, npad, D = q.shape
    hd = D // heads
    out = np.zeros_like(q)
    pos = np.arange(npad)
    if table is not None:
        table = np.asarray(table, np.float64)
        radius = table.shape[1] // 2
        index = np.clip(pos[:, None] - pos[None, :], -radius, radius) + radius
    for b in range(B):
        n = int(lens[b])
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            s = q[b, :, c] @ k[b, :n, c].T
            if table is not None:
                s = s + table[h][index[:, :n]]
            p = np.exp2(s - s.max(-1, keepdims=True))
            out[b, :, c] = ((R.r16(p) if f16 else p) @ v[b, :n, c]) / p.sum(-1, keepdims=True)
    return out


def forward(sd, cfg, ids, lens, buckets=None, mode="mean", normalize=False, f16=False):
    """sd under the family's names -> (taps float64 (depth + 1, B, npad, D), embeddings (B, D)), as bert_text_ref.forward.  Rows
    >= lens[b] take the position row pos_offset + t like any other, as the encoder computes them (transformers gives them the
    pad row; nobody reads them)"""
    rnd = R.r16 if f16 else (lambda x: np.asarray(x, np.float64))
    W = {k: np.asarray(v, np.float64) for k, v in canonical(sd, cfg["family"]).items()}
    D, heads, eps = cfg["dim"], cfg["heads"], cfg["eps"]
    scale = LOG2E / math.sqrt(D // heads)
    ids = np.asarray(ids)
    B, npad = ids.shape
    x = W["embeddings.word_embeddings.weight"][ids]
    if cfg["type_vocab"]:
        x = x + W["embeddings.token_type_embeddings.weight"][0]
    x = x + W["embeddings.position_embeddings.weight"][cfg["pos_offset"]:cfg["pos_offset"] + npad]
    h = R.layer_norm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps)
    table = None
    if cfg["family"] == "mpnet":
        table = rel_table(W["encoder.relative_attention_bias.weight"], buckets) * LOG2E
    taps = [h]
    for n in range(cfg["depth"]):
        p = f"encoder.layer.{n}."
        ht = rnd(h)
        q = rnd(ht @ rnd(W[p + "attention.self.query.weight"] * scale).T + W[p + "attention.self.query.bias"] * scale)
        k = rnd(ht @ rnd(W[p + "attention.self.key.weight"]).T + W[p + "attention.self.key.bias"])
        v = rnd(ht @ rnd(W[p + "attention.self.value.weight"]).T)       # the value bias is added behind the soft-max
        ao = rnd(attention(q, k, v, lens, heads, table, f16))
        wo = W[p + "attention.output.dense.weight"]
        y = ao @ rnd(wo).T + (W[p + "attention.output.dense.bias"] + wo @ W[p + "attention.self.value.bias"]) + h
        h = R.layer_norm(y, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        ht = rnd(h)
        hid = rnd(R.gelu(ht @ rnd(W[p + "intermediate.dense.weight"]).T + W[p + "intermediate.dense.bias"]))
        y = hid @ rnd(W[p + "output.dense.weight"]).T + W[p + "output.dense.bias"] + h
        h = R.layer_norm(y, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
        taps.append(h)
    return np.stack(taps), R.pool(h, lens, mode, normalize)


# ---------------------------------------------------------------------------------------------------- the golden
def stored_rows(lens):
    """(n, 4): the rows of every hidden state that the golden keeps (the pooled outputs pin the rest of the last one)"""
    return np.array([[0, 1, n - 2, n - 1] for n in lens], np.int32)


def stored_rows_long(lens):
    return np.array([[0, 127, 128, n - 1] for n in lens], np.int32)


def take_rows(taps, rows):
    """taps (depth + 1, n, npad, dim), rows (n, 4) -> (depth + 1, n, 4, dim)"""
    return np.asarray(taps)[:, np.arange(len(rows))[:, None], rows]


def load_golden(path=GOLDEN):
    """-> ({name: dict(state, ids, lens, rows, hidden_rows, mean, mean_norm, cls)} for MODELS and "mpnet_b_long" (MPNet-B's
    weights on the long batch, no state of its own), buckets int64 (2 BUCKET_SPAN + 1,), the tokenizer cases)"""
    z = np.load(path)
    models = {}
    for name in list(MODELS) + ["mpnet_b_long"]:
        entry = {k: z[f"{name}/{k}"] for k in ("ids", "lens", "rows", "hidden_rows", "mean", "mean_norm", "cls")}
        if name in MODELS:
            keys = json.loads(str(z[f"{name}/keys"]))
            exps = z[f"{name}/exps"]
            entry["state"] = {k: (z[f"{name}/w{i}"].astype(np.float64) * 2.0 ** int(exps[i])).astype(np.float32) for i, k in enumerate(keys)}
        models[name] = entry
    models["mpnet_b_long"]["state"] = models["mpnet_b"]["state"]
    return models, z["buckets"].astype(np.int64), json.loads(str(z["tokenizers"]))


# ---------------------------------------------------------------------------------------------------- toy vocabularies
# WordPiece, DistilBERT: the pieces of tests/make_bert_text_golden.py.  MPNet: the same pieces behind its own special tokens, in the
# order of the real vocabulary (<s> 0, <pad> 1, </s> 2)
_PIECES = ["the", "invoice", "total", "in", "##voice", "##s", "##ing", "a", "b", "c", "##a", "##b", "##c", "cafe", "café", "resume",
           "re", "##sume", "##sum", "##e", "amount", "due", "date", "of", "to", "pay", "##ment", "##able", "no", "number", "##ber", "num",
           ",", ".", "!", "?", "-", "$", ":", "(", ")", "/", "#", "1", "2", "3", "##1", "##2", "##3", "##0", "0", "12", "50", "##50", "中",
           "文", "日", "本", "The", "Invoice", "TOTAL", "T", "##OTAL", "I", "##nvoice", "é", "##é", "ü", "uber", "über", "x", "##y", "'", "&"]
BERT_VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + _PIECES
MPNET_VOCAB = ["<s>", "<pad>", "</s>", "[UNK]", "<mask>"] + _PIECES
WORDPIECE_TEXTS = ["the invoice total", "The Invoice TOTAL", "THE INVOICES", "invoicing the totals", "Café résumé", "cafe resume resumes",
                   "über uber Über", "total: $12.50!", "amount due (2/3)", "no. #123 - pay", "payment payable", "中文 invoice",
                   "日本の total 中", "the中invoice", "a" * 101 + " total", "xyzzy the qwerty", "number numb num",
                   "in\x00voice\tthe\r\ntotal", "", "   ", "!!!", "pay-ment's & co.", "abc cba aabbcc", "1 12 123 1230 50 150",
                   " the  invoice ", "I'm T", "TOTALS Invoices"]

# byte-level BPE (RoBERTa): the 256 byte symbols, a few merges over "the invoice total ..." and the special tokens
BPE_MERGES = ["Ġ t", "h e", "Ġt he", "i n", "Ġ in", "v o", "i c", "ic e", "vo ice", "Ġin voice", "t o", "Ġ to", "t a", "a l", "Ġto ta",
              "Ġtota l", "Ġ a", "m o", "u n", "Ġa mo", "un t", "Ġamo unt", "Ġ d", "u e", "Ġd ue", "Ġ 1", "Ġ1 2", "5 0", "Ġ p", "a y",
              "Ġp ay", "Ġ n", "Ġn o", "' t", "Ġ Ġ", "in voice", "t he", "r e", "Ġ re", "s u", "m e", "Ġre su", "Ġresu me"]
BPE_TEXTS = ["the invoice total", "The Invoice TOTAL", "invoice the total", " the invoice", "the invoice ", "the  invoice   total",
             "total: $12.50!", "amount due 12 50 1250", "no. #123 - pay", "abc123def 12abc", "don't can't I'm we'll they've it's",
             "Café résumé über", "中文 invoice 日本", "pay 🙂 total 👍🏽", "the\tinvoice\ntotal", "", "   ", "!!!", "pay-ment's & co.",
             "resume resumes to pay the amount due"]


def bpe_vocab():
    """token -> id: the special tokens in RoBERTa's order, the byte alphabet, then every merge's result"""
    from marie_icr_amd.document_classifier import bytes_to_unicode

    tokens = ["<s>", "<pad>", "</s>", "<unk>", "<mask>"] + [bytes_to_unicode()[b] for b in range(256)]
    tokens += [m.replace(" ", "") for m in BPE_MERGES]
    assert len(set(tokens)) == len(tokens)
    return {t: i for i, t in enumerate(tokens)}


def write_bpe_files(directory):
    """vocab.json and merges.txt of the toy byte-level BPE -> their paths"""
    vocab, merges = os.path.join(directory, "vocab.json"), os.path.join(directory, "merges.txt")
    with open(vocab, "w", encoding="utf-8") as f:
        json.dump(bpe_vocab(), f, ensure_ascii=False)
    with open(merges, "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(BPE_MERGES) + "\n")
    return vocab, merges
