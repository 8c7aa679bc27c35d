"""Writes tests/golden/bert_text.npz: what transformers computes for two tiny BERT models and a tiny WordPiece vocabulary, the
third-party pin of tests/bert_text_ref.py and marie_icr_amd/wordpiece_tokenizer.py.

    python tests/make_bert_text_golden.py            (CPU, float64; the file regenerates byte for byte)

Models: transformers.BertModel(add_pooling_layer=False, output_hidden_states=True) in float64 at config A (dim 64, 2 heads of 32,
2 layers, ffn 256) and config B (dim 128, 2 heads of 64), vocabulary 80, 128 positions, eps 1e-12, weights re-drawn by
bert_text_ref.make_state (the default std-0.02 initialisation hides errors) and put on an int8 x 2^e grid so that the file stays
under 1 MB.  Stored: the weights, ids, lengths, every hidden state, and the pooled outputs (masked mean, that normalised, [CLS]).
Tokenizer: transformers.BertTokenizer over a vocabulary of 80 pieces, cased and uncased, on strings that cover case, accents,
punctuation, CJK, control characters, an over-long word, special tokens and unknown pieces.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_text.npz")
LENS, NPAD = [3, 16, 17, 24], 24

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "invoice", "total", "in", "##voice", "##s", "##ing", "a", "b", "c",
         "##a", "##b", "##c", "cafe", "café", "resume", "re", "##sume", "##sum", "##e", "amount", "due", "date", "of", "to", "pay",
         "##ment", "##able", "no", "number", "##ber", "num", ",", ".", "!", "?", "-", "$", ":", "(", ")", "/", "#", "1", "2", "3",
         "##1", "##2", "##3", "##0", "0", "12", "50", "##50", "中", "文", "日", "本", "The", "Invoice", "TOTAL", "T", "##OTAL", "I",
         "##nvoice", "é", "##é", "ü", "uber", "über", "##ber", "x", "##y", "'", "&"]
TEXTS = ["the invoice total", "The Invoice TOTAL", "THE INVOICES", "invoicing the totals", "Café résumé", "cafe resume resumes",
         "über uber Über", "total: $12.50!", "amount due (2/3)", "no. #123 - pay", "payment payable", "中文 invoice", "日本の total 中",
         "the中invoice", "a" * 101 + " total", "a" * 100, "xyzzy the qwerty", "number numb num", "in\x00voice\tthe\r\ntotal",
         "the invoice total", "[MASK] the [SEP] total", "[CLS]invoice", "", "   ", "!!!", "pay-ment's & co.",
         "abc cba aabbcc", "re sume resum", "1 12 123 1230 50 150", "the\ufffdinvoice \u200btotal", "I'm T", "TOTALS Invoices"]


def hf_model(cfg, sd):
    from transformers import BertConfig, BertModel

    conf = BertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["dim"], num_hidden_layers=cfg["depth"], num_attention_heads=cfg["heads"],
                      intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_position"], type_vocab_size=cfg["type_vocab"],
                      layer_norm_eps=cfg["eps"], hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = BertModel(conf, add_pooling_layer=False).double().eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return model


def model_entries(name, cfg, seed):
    sd, packed = R.quantize_state(R.make_state(cfg, seed))
    ids = R.make_ids(cfg, LENS, NPAD, seed)
    mask = R.valid_rows(LENS, NPAD)
    with torch.no_grad():
        out = hf_model(cfg, sd)(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long(),
                                output_hidden_states=True)
    hidden = torch.stack(out.hidden_states)
    assert hidden.shape == (cfg["depth"] + 1, len(LENS), NPAD, cfg["dim"]) and torch.equal(hidden[-1], out.last_hidden_state)
    for i, h in enumerate(hidden):
        top = float(h[torch.from_numpy(mask)].abs().max())
        print(f"config {name}: hidden state {i} reaches {top:.2f}")
        assert 0.5 <= top <= 10, "the hidden states are not O(1)"
    # sentence_transformers' Pooling (mean over the attention mask, or the first token) and Normalize
    m = torch.from_numpy(mask).double()[..., None]
    mean = (hidden[-1] * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
    entries = {f"{name}/keys": np.array(json.dumps(list(packed))), f"{name}/exps": np.array([e for _, e in packed.values()], np.int8),
               f"{name}/ids": ids, f"{name}/lens": np.array(LENS, np.int32), f"{name}/hidden": hidden.numpy(),
               f"{name}/mean": mean.numpy(), f"{name}/mean_norm": torch.nn.functional.normalize(mean, p=2, dim=1).numpy(),
               f"{name}/cls": hidden[-1][:, 0].numpy()}
    for i, (q, _) in enumerate(packed.values()):
        entries[f"{name}/w{i}"] = q
    return entries


def tokenizer_entries():
    from transformers import BertTokenizer

    vocab = list(dict.fromkeys(VOCAB))
    cases = {}
    for lower in (True, False):
        tok = BertTokenizer(vocab={v: i for i, v in enumerate(vocab)}, do_lower_case=lower)
        cases["uncased" if lower else "cased"] = [tok(t)["input_ids"] for t in TEXTS]
    print(f"tokenizer: {len(vocab)} pieces, {len(TEXTS)} strings, "
          f"{sum(ids.count(1) for ids in cases['uncased'])} unknown pieces (uncased)")
    return {"tokenizer": np.array(json.dumps(dict(vocab=vocab, texts=TEXTS, ids=cases)))}


def write_npz(path, entries):
    """an .npz whose bytes depend on the arrays alone (np.savez stamps the time of writing into the archive)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(entries):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(entries[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    entries = {}
    entries.update(model_entries("A", R.CONFIG_A, 11))
    entries.update(model_entries("B", R.CONFIG_B, 12))
    entries.update(tokenizer_entries())
    write_npz(OUT, entries)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    main()
