"""Times the Longformer page classifier (f16): python tools/time_text_classifier.py [--pages 32] [--repeats 5]

Seeded random weights at the longformer-base-4096 shape (768 / 12 heads of 64 / 12 layers / ffn 3072, attention_window 512, 4098
position rows, 3 labels) over the toy byte-level BPE of tests/sentence_families_ref.py; `--pages` pages of 3000 to 4096 tokens.

  * `predict`: TransformersDocumentClassifier(task="text-classification").predict — the host tokenizer, the length buckets, per
    bucket ids up, the model, logits and scores back;
  * `classify`: the model calls alone on the same buckets, ids already tokenized and padded;
  * in a pass of its own (the events slow the host), the device time per kernel family from the context's profiler; attn_window and
    attn_global_row are counted in its `attn_short` slot, whose share is reported as "attn_share";
  * `window_vs_long`: attn_window (w = 256) and attn_long on the same q, k, v — `--cmp-texts` texts of 4096 rows, 12 heads — device
    time of each from the profiler.  The band has (2 * 256 + 2) / 4096 of the keys; in staged key tiles about a sixth.

Each wall figure is the median of `--repeats` windows of at least `--window` seconds after `--warmup` warm calls; min and max are
reported with it.  Prints one JSON line.  Nothing is asserted on these numbers; this is not bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BASE = dict(max_position=4098, type_vocab=1, dim=768, heads=12, depth=12, ffn=3072, eps=1e-5, position="absolute", mlp="gelu",
            attention_window=512, num_labels=3, logit_gain=2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds of one timed window")
    ap.add_argument("--cmp-texts", type=int, default=4)
    args = ap.parse_args()

    import longformer_ref as L
    import sentence_families_ref as S
    from time_text_embeddings import IGEMM_TILE_SLOTS, clocks, timed

    from marie_icr_amd import embeddings, text_classifier
    from marie_icr_amd._lib import PREC_F16, Context
    from marie_icr_amd.document_classifier import TransformersDocumentClassifier

    ctx = Context(0)
    cfg = dict(BASE, vocab=L.VOCAB)
    result = {"precision": "f16", "device": ctx.device_info(), "clocks": clocks(), "pages": args.pages,
              "dim_heads_depth_ffn": [cfg["dim"], cfg["heads"], cfg["depth"], cfg["ffn"]], "attention_window": cfg["attention_window"]}
    rng = np.random.default_rng(0)
    words = [[L._WORDS[j] for j in rng.integers(0, len(L._WORDS), c)] for c in rng.integers(1700, 2300, args.pages)]
    with tempfile.TemporaryDirectory() as d:
        S.write_bpe_files(d)
        clf = TransformersDocumentClassifier(d, task="text-classification", top_k=3, state=L.make_state(cfg, 0), config=L.config_json(cfg),
                                             precision="f16", ctx=ctx, batch_size=64)
    tm = clf.text_model
    encoded = [tm.encode(" ".join(w)) for w in words]
    lengths = [len(e) for e in encoded]
    groups = [tm.tokenizer.pad([encoded[i] for i in members], npad)
              for npad, members in embeddings.plan_text_groups(lengths, tm.TEXT_CHUNK, tm._rows_budget())]
    whole = timed(lambda: clf.predict(words, words), args.warmup, args.repeats, args.window)
    device = timed(lambda: [tm.model.classify_ids_host(ids, lens) for ids, lens in groups], args.warmup, args.repeats, args.window)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for ids, lens in groups:
        tm.model.classify_ids_host(ids, lens)
    prof = {k: round(v["total_ms"], 3) for k, v in ctx.profile_read().items() if v["launches"] and v["id"] not in IGEMM_TILE_SLOTS}
    ctx.profile_enable(False)
    out = clf.predict(words[:4], words[:4])
    result.update({
        "tokens": [min(lengths), max(lengths)], "tokens_total": int(sum(lengths)), "calls": len(groups),
        "rows_per_page_by_call": [int(ids.shape[1]) for ids, _ in groups],
        "predict": {"pages_per_s": round(args.pages / whole[0], 2), "ms": round(whole[0] * 1e3, 2),
                    "ms_min_max": [round(whole[1] * 1e3, 2), round(whole[2] * 1e3, 2)], "calls_per_window": whole[3]},
        "classify": {"pages_per_s": round(args.pages / device[0], 2), "ms": round(device[0] * 1e3, 2),
                     "ms_min_max": [round(device[1] * 1e3, 2), round(device[2] * 1e3, 2)]},
        "device_ms_by_kernel_family": prof, "device_ms_total": round(sum(prof.values()), 3),
        "attn_share": round(prof.get("attn_short", 0.0) / max(sum(prof.values()), 1e-9), 4),
        "first_labels": [o["label"] for o in out], "finite": bool(all(np.isfinite(o["score"]) for o in out))})
    clf.close()

    # the kernel against the full streamed attention on the same rows
    B, npad, heads = args.cmp_texts, 4096, 12
    qrng = np.random.default_rng(1)
    q = (qrng.standard_normal((B, npad, heads * 64)) * (L.LOG2E / 8)).astype(np.float32)
    k = qrng.standard_normal((B, npad, heads * 64)).astype(np.float32)
    v = qrng.standard_normal((B, npad, heads * 64)).astype(np.float32)
    lens = np.full(B, npad, np.int32)
    cmp = {}
    for name, fn in (("attn_window", lambda: text_classifier.window_attention_host(ctx, PREC_F16, q, k, v, lens, heads, 256)),
                     ("attn_long", lambda: embeddings.long_attention_host(ctx, PREC_F16, q, k, v, lens, heads))):
        fn()
        ms = []
        for _ in range(args.repeats):
            ctx.profile_enable(True)
            ctx.profile_reset()
            fn()
            ms.append(ctx.profile_read()["attn_short"]["total_ms"])
            ctx.profile_enable(False)
        cmp[name] = {"device_ms": round(float(np.median(ms)), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}
    cmp["texts_rows_heads"] = [B, npad, heads]
    cmp["ratio_long_over_window"] = round(cmp["attn_long"]["device_ms"] / max(cmp["attn_window"]["device_ms"], 1e-9), 2)
    result["window_vs_long"] = cmp
    print(json.dumps(result))


if __name__ == "__main__":
    main()
