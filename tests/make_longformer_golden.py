"""Writes tests/golden/longformer.npz: what transformers computes for two tiny LongformerForSequenceClassification models and
LongformerTokenizer over the toy byte-level BPE of sentence_families_ref — the third-party pin of tests/longformer_ref.py, of the
tokenisation and truncation in marie_icr_amd/text_classifier.py and of the classifier's labels and scores.

    python tests/make_longformer_golden.py            (CPU, float64; the file regenerates byte for byte)

Models (longformer_ref.MODELS): A with attention_window [16, 48] and three labels, B with the window 32 and one label; hidden 128,
2 heads of 64, 2 layers, ffn 256, float64, seeded O(1) weights on an int8 x 2^e grid, out_proj scaled by logit_gain.  The weights are
not stored: longformer_ref.make_state regenerates them from the seed.  Texts (longformer_ref.TEXT_TOKENS): 13 of 2 .. 230 tokens,
the longest cut to model_max_length = 192 by truncation=True.  Every text goes through the model alone, with no global attention
mask, as pipeline("text-classification") calls it; the library pads it to a multiple of the window itself.  Stored: the texts, the
tokenizer's ids, four rows a text of every hidden state, the logits and the pipeline's scores (its own softmax / sigmoid).
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import longformer_ref as L  # noqa: E402
import sentence_families_ref as S  # noqa: E402
from make_bert_text_golden import write_npz  # noqa: E402


def hf_tokenizer():
    from transformers import LongformerTokenizer

    return LongformerTokenizer(vocab=S.bpe_vocab(), merges=[tuple(m.split(" ")) for m in S.BPE_MERGES], model_max_length=L.MODEL_MAX_LENGTH)


def hf_model(cfg, sd):
    import transformers as T

    conf = T.LongformerConfig(vocab_size=cfg["vocab"], max_position_embeddings=cfg["max_position"], hidden_size=cfg["dim"],
                              num_attention_heads=cfg["heads"], num_hidden_layers=cfg["depth"], intermediate_size=cfg["ffn"],
                              layer_norm_eps=cfg["eps"], hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                              pad_token_id=1, bos_token_id=0, eos_token_id=2, sep_token_id=2, type_vocab_size=cfg["type_vocab"],
                              attention_window=cfg["attention_window"], num_labels=cfg["num_labels"])
    model = T.LongformerForSequenceClassification(conf).double().eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") or k.endswith("token_type_ids") for k in missing), (missing, unexpected)
    return model


def pipeline_scores(logits, cfg):
    from transformers.pipelines.text_classification import sigmoid, softmax

    return sigmoid(logits) if cfg["num_labels"] == 1 else softmax(logits)


def model_entries(name, ids):
    cfg = L.MODELS[name]
    model = hf_model(cfg, L.make_state(cfg, L.SEEDS[name]))
    rows = L.stored_rows([len(e) for e in ids])
    tap_rows, logits = [], []
    for i, e in enumerate(ids):
        with torch.no_grad():
            out = model(input_ids=torch.tensor([list(e)]).long(), output_hidden_states=True)
        hidden = torch.stack(out.hidden_states)[:, 0, :len(e)].numpy()      # the library's own padding rows dropped
        assert hidden.shape == (cfg["depth"] + 1, len(e), cfg["dim"])
        top = float(np.abs(hidden).max())
        assert 0.5 <= top <= 12, f"the hidden states are not O(1): {top}"
        tap_rows.append(hidden[:, rows[i]])
        logits.append(out.logits[0].numpy())
    logits = np.stack(logits)
    scores = np.stack([pipeline_scores(z, cfg) for z in logits])
    print(f"{name}: logits reach {np.abs(logits).max():.2f}; labels {logits.argmax(-1).tolist()}; top scores {np.round(scores.max(-1), 3).tolist()}")
    return {f"{name}/tap_rows": np.stack(tap_rows, 1), f"{name}/logits": logits, f"{name}/scores": scores}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    tok = hf_tokenizer()
    texts = L.make_texts(lambda t: len(tok(t)["input_ids"]))
    ids = [np.array(tok(t, truncation=True)["input_ids"], np.int32) for t in texts]
    lens = [len(e) for e in ids]
    print("token counts:", lens)
    assert lens == [min(n, L.MODEL_MAX_LENGTH) for n in L.TEXT_TOKENS], lens
    assert all(e[0] == 0 and e[-1] == 2 and 1 not in e for e in ids)
    entries = {"texts": np.array(json.dumps(texts)), "lens": np.array(lens, np.int32), "ids": np.concatenate(ids).astype(np.int16)}
    for name in L.MODELS:
        entries.update(model_entries(name, ids))
    write_npz(L.GOLDEN, entries)
    print(f"{L.GOLDEN}: {os.path.getsize(L.GOLDEN)} bytes")
    assert os.path.getsize(L.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
