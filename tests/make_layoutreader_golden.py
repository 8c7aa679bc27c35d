"""Writes tests/golden/layoutreader.npz: what the LayoutReader model itself computes for a tiny configuration, the third-party
pin of tests/layoutreader_ref.py.

    python tests/make_layoutreader_golden.py <checkout of marie-ai>      (CPU, float64; the file regenerates byte for byte)

The model is LayoutlmForSeq2SeqDecoder of marie/models/unilm/layoutreader/s2s_ft/modeling_decoding.py, loaded by file path (the
file needs torch alone; its apex import is optional), greedy (search_beam_size 1, pos_shift off), layoutlm_only_layout_flag set,
in float64.  Its inputs are laid out as Preprocess4Seq2seqDecoder lays them out (that class pads to 511 words whatever it is
told, so the layout is restated here for S source rows): ids [S][5], type ids, position ids and the [S + T][S + T] mask.

Configuration: layoutreader_ref.CONFIG (dim 128, 2 heads of 64, 2 layers, ffn 256, S = 34, T = 32), pages of 1, 9, 17 and 32
words (layoutreader_ref.make_pages), weights of layoutreader_ref.make_state on the int8 x 2^e grid.  Stored: the weights, the
boxes, every step's decision and score row (hooked at cls.predictions) and the embedded source rows the head scores against.
The smallest top-2 margin over the 128 steps is printed and must be >= 0.05 (a seed that quantises below that is redrawn).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layoutreader_ref as R  # noqa: E402
from make_bert_text_golden import write_npz  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layoutreader.npz")
MODEL_FILE = os.path.join("marie", "models", "unilm", "layoutreader", "s2s_ft", "modeling_decoding.py")


def load_model_module(checkout):
    spec = importlib.util.spec_from_file_location("layoutreader_modeling_decoding", os.path.join(checkout, MODEL_FILE))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_model(M, cfg, sd):
    conf = M.BertConfig(30522, hidden_size=cfg["dim"], num_hidden_layers=cfg["depth"], num_attention_heads=cfg["heads"],
                        intermediate_size=cfg["ffn"], hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        max_position_embeddings=cfg["max_position"], type_vocab_size=cfg["type_vocab"],
                        source_type_id=cfg["source_type"], target_type_id=cfg["target_type"])
    conf.layoutlm_only_layout_flag = True
    conf.max_2d_position_embeddings = cfg["max_2d"]
    conf.base_model_type = "layoutlm"
    conf.max_source_length = cfg["max_source"]
    model = M.LayoutlmForSeq2SeqDecoder(conf, mask_word_id=103, search_beam_size=1, eos_id=102, sos_id=102, mode="s2s", pos_shift=False)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith(("bert.pooler.", "cls.seq_relationship.")) for k in missing), (missing, unexpected)
    return model.double().eval()


def model_inputs(cfg, boxes):
    """one page as Preprocess4Seq2seqDecoder + batch_list_to_batch_tensors hand it to the model"""
    S, n = cfg["max_source"], len(boxes)
    T = S - 2
    rows, pos = R.source_rows(cfg, boxes)
    ids = np.zeros((S, 5), np.int64)
    ids[:, 0] = [101] + [1996] * n + [102] + [0] * (S - n - 2)      # never embedded
    ids[:, 1:] = rows
    types = [cfg["source_type"]] * S + [cfg["target_type"]] * T
    position = list(pos) + [i - S + n + 2 for i in range(S, S + T)]
    mask = torch.zeros(S + T, S + T, dtype=torch.long)
    mask[:, :n + 2] = 1
    mask[S:, S:] = torch.tril(torch.ones(T, T, dtype=torch.long))
    return (torch.from_numpy(ids)[None], torch.tensor(types)[None], torch.tensor(position)[None], mask[None])


def run_model(model, cfg, boxes):
    steps, emb = [], []

    def hook(_module, inputs, output):
        steps.append(output[0, 0].clone())
        emb.append(inputs[1][0].clone())

    handle = model.cls.predictions.register_forward_hook(hook)
    with torch.no_grad():
        out = model(*model_inputs(cfg, boxes))
    handle.remove()
    scores = torch.stack(steps).numpy()
    assert scores.shape == (cfg["max_source"] - 2, cfg["max_source"]) and all(torch.equal(e, emb[0]) for e in emb)
    decisions = out[0].numpy().astype(np.int32)
    assert np.array_equal(decisions, scores.argmax(-1))
    return decisions, scores, emb[0].numpy()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    cfg = R.CONFIG
    M = load_model_module(sys.argv[1])
    sd, packed = R.quantize_state(R.make_state(cfg, R.SEED))
    model = build_model(M, cfg, sd)
    pages = R.make_pages(cfg, R.SEED)
    S = cfg["max_source"]
    boxes = np.zeros((len(pages), S - 2, 4), np.int32)
    decisions, scores, emb = [], [], []
    for i, b in enumerate(pages):
        boxes[i, :len(b)] = b
        d, s, e = run_model(model, cfg, b)
        decisions.append(d), scores.append(s), emb.append(e)
        print(f"page of {len(b)} words: {len(set(d.tolist()))} distinct decisions {sorted(set(d.tolist()))}, "
              f"scores within +-{np.abs(s).max():.1f}")
    scores = np.stack(scores)
    m = R.margins(scores).ravel()
    print(f"top-2 margins over {m.size} steps: min {m.min():.3f}, median {np.median(m):.2f}, "
          f"{(m < 0.2).mean():.0%} < 0.2, {(m < 0.5).mean():.0%} < 0.5, {(m < 0.9).mean():.0%} < 0.9")
    assert m.min() >= 0.05, "a margin below 0.05: redraw layoutreader_ref.SEED"
    entries = {"config": np.array(json.dumps(cfg)), "keys": np.array(json.dumps(list(packed))),
               "exps": np.array([e for _, e in packed.values()], np.int8), "boxes": boxes,
               "counts": np.array([len(b) for b in pages], np.int32), "decisions": np.stack(decisions), "scores": scores,
               "emb": np.stack(emb)}
    for i, (q, _) in enumerate(packed.values()):
        entries[f"w{i}"] = q
    write_npz(OUT, entries)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    main()
