"""Writes tests/golden/sentence_families.npz: what transformers computes for tiny MPNet, RoBERTa and DistilBERT models and their
tokenizers over toy vocabularies, the third-party pin of tests/sentence_families_ref.py, of the loader and tokenizers in
marie_icr_amd and of mhip_berttext_rel_table.

    python tests/make_sentence_families_golden.py            (CPU, float64; the file regenerates byte for byte)

Models (sentence_families_ref.MODELS): MPNetModel at dim 64 / 2 heads of 32 (136 positions) and dim 128 / 2 heads of 64 (520
positions), RobertaModel at dim 128 (one token type, 136 positions), DistilBertModel at dim 64; two layers each, no pooler,
float64, weights re-drawn at O(1) scale and put on an int8 x 2^e grid.  Batch: lengths 3, 16, 17, 24 in 24 rows; the larger MPNet
also on lengths 129, 131, 257 in 264 rows (distances past the bias table's 128 on both sides, three key blocks).  Stored: the
weights, ids, lengths, four rows a text of every hidden state (the first two and last two tokens; 0, 127, 128 and the last of
the long batch) and the pooled outputs (masked mean, that normalised, the first token), which pin every row of the last state.
Also MPNetEncoder.relative_position_bucket(rel, 32, 128) for rel in -600 .. 600, and the ids MPNetTokenizer, RobertaTokenizer and
DistilBertTokenizer give on the strings of sentence_families_ref.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bert_text_ref as R  # noqa: E402
import sentence_families_ref as S  # noqa: E402
from make_bert_text_golden import write_npz  # noqa: E402


def hf_model(cfg, sd):
    import transformers as T

    family = cfg["family"]
    common = dict(vocab_size=cfg["vocab"], max_position_embeddings=cfg["max_position"])
    if family == "distilbert":
        conf = T.DistilBertConfig(dim=cfg["dim"], n_heads=cfg["heads"], n_layers=cfg["depth"], hidden_dim=cfg["ffn"], activation="gelu",
                                  dropout=0.0, attention_dropout=0.0, sinusoidal_pos_embds=False, pad_token_id=0, **common)
        model = T.DistilBertModel(conf)
    else:
        args = dict(hidden_size=cfg["dim"], num_attention_heads=cfg["heads"], num_hidden_layers=cfg["depth"], intermediate_size=cfg["ffn"],
                    layer_norm_eps=cfg["eps"], hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                    pad_token_id=1, **common)
        if family == "mpnet":
            model = T.MPNetModel(T.MPNetConfig(relative_attention_num_buckets=S.REL_BUCKETS, **args), add_pooling_layer=False)
        else:
            model = T.RobertaModel(T.RobertaConfig(type_vocab_size=cfg["type_vocab"], **args), add_pooling_layer=False)
    model = model.double().eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") or k.endswith("token_type_ids") for k in missing), (missing, unexpected)
    return model


def batch_entries(name, cfg, model, lens, npad, seed, rows):
    ids = S.make_ids(cfg, lens, npad, seed)
    mask = R.valid_rows(lens, npad)
    with torch.no_grad():
        out = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long(), output_hidden_states=True)
    hidden = torch.stack(out.hidden_states)
    assert hidden.shape == (cfg["depth"] + 1, len(lens), npad, cfg["dim"]) and torch.equal(hidden[-1], out.last_hidden_state)
    for i, h in enumerate(hidden):
        top = float(h[torch.from_numpy(mask)].abs().max())
        print(f"{name}: hidden state {i} reaches {top:.2f}")
        assert 0.5 <= top <= 10, "the hidden states are not O(1)"
    m = torch.from_numpy(mask).double()[..., None]
    mean = (hidden[-1] * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
    return {f"{name}/ids": ids, f"{name}/lens": np.array(lens, np.int32), f"{name}/rows": rows,
            f"{name}/hidden_rows": S.take_rows(hidden.numpy(), rows), f"{name}/mean": mean.numpy(),
            f"{name}/mean_norm": torch.nn.functional.normalize(mean, p=2, dim=1).numpy(), f"{name}/cls": hidden[-1][:, 0].numpy()}


def model_entries(name):
    cfg, seed = S.MODELS[name], S.SEEDS[name]
    sd, packed = R.quantize_state(S.make_state(cfg, seed))
    model = hf_model(cfg, sd)
    entries = {f"{name}/keys": np.array(json.dumps(list(packed))), f"{name}/exps": np.array([e for _, e in packed.values()], np.int8)}
    for i, (q, _) in enumerate(packed.values()):
        entries[f"{name}/w{i}"] = q
    entries.update(batch_entries(name, cfg, model, S.LENS, S.NPAD, seed, S.stored_rows(S.LENS)))
    if name == "mpnet_b":
        entries.update(batch_entries("mpnet_b_long", cfg, model, S.LONG_LENS, S.LONG_NPAD, seed + 100, S.stored_rows_long(S.LONG_LENS)))
    return entries


def bucket_entries():
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder

    rel = torch.arange(-S.BUCKET_SPAN, S.BUCKET_SPAN + 1, dtype=torch.long)
    buckets = MPNetEncoder.relative_position_bucket(rel, num_buckets=S.REL_BUCKETS, max_distance=S.REL_MAX_DISTANCE).numpy()
    assert buckets.min() == 0 and buckets.max() == S.REL_BUCKETS - 1
    return {"buckets": buckets.astype(np.int16)}


def tokenizer_entries():
    from transformers import DistilBertTokenizer, MPNetTokenizer, RobertaTokenizer

    cases = {}
    for lower in (True, False):
        which = "uncased" if lower else "cased"
        tok = MPNetTokenizer(vocab={v: i for i, v in enumerate(S.MPNET_VOCAB)}, do_lower_case=lower)
        cases[f"mpnet_{which}"] = [tok(t)["input_ids"] for t in S.WORDPIECE_TEXTS]
        tok = DistilBertTokenizer(vocab={v: i for i, v in enumerate(S.BERT_VOCAB)}, do_lower_case=lower)
        cases[f"distilbert_{which}"] = [tok(t)["input_ids"] for t in S.WORDPIECE_TEXTS]
    tok = RobertaTokenizer(vocab=S.bpe_vocab(), merges=[tuple(m.split(" ")) for m in S.BPE_MERGES])
    cases["roberta"] = [tok(t)["input_ids"] for t in S.BPE_TEXTS]
    print(f"tokenizers: {len(S.WORDPIECE_TEXTS)} WordPiece strings, {len(S.BPE_TEXTS)} BPE strings, "
          f"{sum(len(i) for i in cases['roberta'])} BPE ids")
    return {"tokenizers": np.array(json.dumps(cases))}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    entries = {}
    for name in S.MODELS:
        entries.update(model_entries(name))
    entries.update(bucket_entries())
    entries.update(tokenizer_entries())
    write_npz(S.GOLDEN, entries)
    print(f"{S.GOLDEN}: {os.path.getsize(S.GOLDEN)} bytes")
    assert os.path.getsize(S.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
