"""Writes tests/golden/bert_text_long.npz: what transformers computes for the two tiny BERT models of tests/make_bert_text_golden.py
with 512 positions on texts past 128 tokens, the third-party pin of tests/bert_text_ref.py at the lengths the streamed attention
(attn_long, marie_icr_amd/csrc/attn_seq.hip) serves.

    python tests/make_bert_text_long_golden.py            (CPU, float64; the file regenerates byte for byte)

Models: transformers.BertModel(add_pooling_layer=False, output_hidden_states=True) in float64 at bert_text_ref.CONFIG_A and
CONFIG_B with max_position 512, weights from make_state / quantize_state (seeds 21, 22).  Texts of 129, 257 and 512 tokens at npad
512.  Stored: the packed weights, ids, lengths, the pooled outputs (masked mean, that normalised, [CLS]) and, of every hidden state,
the rows 0, 127, 128 and len - 1 of each text (`hidden_rows`, (depth + 1, 3, 4, dim); `rows` (3, 4) names them) — full hidden
states would not fit under the size limit of a committed file.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402
from make_bert_text_golden import hf_model, write_npz  # noqa: E402
from bert_text_long import CONFIG_A, CONFIG_B, GOLDEN as OUT, LENS, NPAD, stored_rows  # noqa: E402


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
    m = torch.from_numpy(mask).double()[..., None]
    mean = (hidden[-1] * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
    rows = stored_rows(LENS)
    kept = hidden.numpy()[:, np.arange(len(LENS))[:, None], rows]      # (depth + 1, n, 4, dim)
    entries = {f"{name}/keys": np.array(json.dumps(list(packed))), f"{name}/exps": np.array([e for _, e in packed.values()], np.int8),
               f"{name}/ids": ids, f"{name}/lens": np.array(LENS, np.int32), f"{name}/rows": rows, f"{name}/hidden_rows": kept,
               f"{name}/mean": mean.numpy(), f"{name}/mean_norm": torch.nn.functional.normalize(mean, p=2, dim=1).numpy(),
               f"{name}/cls": hidden[-1][:, 0].numpy()}
    for i, (q, _) in enumerate(packed.values()):
        entries[f"{name}/w{i}"] = q
    return entries


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    entries = {}
    entries.update(model_entries("A", CONFIG_A, 21))
    entries.update(model_entries("B", CONFIG_B, 22))
    write_npz(OUT, entries)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    main()
