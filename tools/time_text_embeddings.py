"""Times the BERT sentence encoders (f16): python tools/time_text_embeddings.py [--texts 4096] [--repeats 7] [--shapes minilm jina]
                                                                                  [--legs short long]
(more shapes: mpnet bertbase distilroberta, short leg only)

Seeded random weights at the all-MiniLM-L6-v2 shape (384 / 12 heads of 32 / 6 layers / ffn 1536, position table, GELU, mean +
normalize) and the jina-embeddings-v2-base-en shape (768 / 12 heads of 64 / 12 layers / ffn 3072, ALiBi, GEGLU, mean), a synthetic
WordPiece vocabulary of one-piece words.  Also the all-mpnet-base-v2 shape (`mpnet`: 768 / 12 heads of 64 / 12 layers / ffn 3072,
514 position rows from row 2, no token types, the relative attention bias), a BERT-base-shaped model of the same geometry
(`bertbase`: what `mpnet` costs without the table term) and the all-distilroberta-v1 shape (`distilroberta`: the same with 6
layers, one token type, no bias); all three over the same WordPiece words (a tokenizer handed to the class), since the encoder is
what is timed.  The short leg: `--texts` texts of 4 to 24 tokens ([CLS] and [SEP] included), which run
through attn_short.  The long leg (result key "long_shapes"): 256 texts of 200 to 256 tokens at the MiniLM shape and 64 texts of 400
to 512 tokens at the jina shape, which run through the streamed attn_long (both kernels are counted in the profiler's `attn_short`
slot; its share of the device time is reported as "attn_share").  Per shape and leg:

  * `embed_texts`: what `MetaTemplateMatcher.text_sims` calls — the host tokenizer, the length-bucketed groups, per group ids up,
    the encoder, the embeddings back, ending in a stream synchronise.  The same texts are embedded again and again, so the
    tokenizer finds the ids of every word remembered; the figure beside it clears that memory before every call;
  * the encoder calls alone on the same groups, ids already tokenized and padded;
  * in a pass of its own (the events slow the host), the device time per kernel family from the context's profiler (device events
    around every launch).

Each figure is the median of `--repeats` windows of at least `--window` seconds after `--warmup` warm calls; min and max are
reported with it.  The clocks `rocm-smi --showclocks` reports at the start are noted (read only).  Prints one JSON line.  Nothing
is asserted on these numbers; this is not bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {
    "minilm": dict(vocab=30522, max_position=512, type_vocab=2, dim=384, heads=12, depth=6, ffn=1536, eps=1e-12, position="absolute",
                   mlp="gelu", cls="SentenceTransformerEmbeddings"),
    "jina": dict(vocab=30528, max_position=8192, type_vocab=2, dim=768, heads=12, depth=12, ffn=3072, eps=1e-12, position="alibi",
                 mlp="geglu", cls="JinaEmbeddings"),
    "bertbase": dict(vocab=30527, max_position=514, type_vocab=2, dim=768, heads=12, depth=12, ffn=3072, eps=1e-12, position="absolute",
                     mlp="gelu", cls="SentenceTransformerEmbeddings"),
    # the other families: weights and config.json from tests/sentence_families_ref.py
    "mpnet": dict(family="mpnet", vocab=30527, max_position=514, type_vocab=0, dim=768, heads=12, depth=12, ffn=3072, eps=1e-5, pos_offset=2,
                  position="absolute", mlp="gelu", cls="SentenceTransformerEmbeddings"),
    "distilroberta": dict(family="roberta", vocab=50265, max_position=514, type_vocab=1, dim=768, heads=12, depth=6, ffn=3072, eps=1e-5,
                          pos_offset=2, position="absolute", mlp="gelu", cls="SentenceTransformerEmbeddings"),
}
LONG_LEG = {"minilm": (256, 200, 256), "jina": (64, 400, 512)}      # texts, fewest and most tokens of one


# profiler slots 12 .. 16 (MHIP_K_IGEMM_T64 .. MHIP_K_IGEMM_PATCH) are conv_igemm by tile shape: their launches are also counted in
# the parent slot "conv_igemm", so a sum over all slots would count the GEMMs twice
IGEMM_TILE_SLOTS = range(12, 17)


def timed(fn, warmup: int, repeats: int, window: float):
    """median seconds per call over `repeats` windows of >= `window` seconds (each call ends in a device synchronise)"""
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    fn()
    calls = max(1, int(window / max(time.perf_counter() - t0, 1e-6)))
    per_call = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        per_call.append((time.perf_counter() - t0) / calls)
    return statistics.median(per_call), min(per_call), max(per_call), calls


def clocks() -> str:
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        lines = [" ".join(ln.split()) for ln in out.splitlines() if "clk" in ln.lower() and "level" in ln.lower()]
        return "; ".join(lines) or "not read"
    except Exception as e:  # noqa: BLE001
        return f"not read ({type(e).__name__})"


def gflop_per_row(cfg) -> float:
    """the GEMMs of one token row: q, k, v, output projection and the MLP (three F x D matrices when gated), 2 FLOP per MAC"""
    D, F = cfg["dim"], cfg["ffn"]
    return cfg["depth"] * 2.0 * (4 * D * D + (3 if cfg["mlp"] == "geglu" else 2) * D * F) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=4096)
    ap.add_argument("--shapes", nargs="+", default=["minilm", "jina"], choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds of one timed window")
    ap.add_argument("--legs", nargs="+", default=["short", "long"], choices=["short", "long"])
    args = ap.parse_args()

    import bert_text_ref as R
    import sentence_families_ref as S
    from marie_icr_amd import embeddings
    from marie_icr_amd._lib import Context
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    ctx = Context(0)
    result = {"precision": "f16", "device": ctx.device_info(), "clocks": clocks(), "texts": args.texts, "tokens_per_text": [4, 24],
              "shapes": {}, "long_shapes": {}}
    words = [f"w{i}" for i in range(2000)]
    tok = WordPieceTokenizer(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words)
    rng = np.random.default_rng(0)
    texts = [" ".join(words[j] for j in rng.integers(0, len(words), c)) for c in rng.integers(2, 23, args.texts)]
    legs = []
    for name in args.shapes:
        if "short" in args.legs:
            legs.append((name, "shapes", texts))
        if "long" in args.legs and name in LONG_LEG:
            n, lo, hi = LONG_LEG[name]
            lrng = np.random.default_rng(1)
            legs.append((name, "long_shapes", [" ".join(words[j] for j in lrng.integers(0, len(words), c)) for c in lrng.integers(lo - 2, hi - 1, n)]))
    for name, leg, texts in legs:
        cfg = SHAPES[name]
        if "family" in cfg:
            state, conf = S.make_state(cfg, 0), S.config_json(cfg)
        else:
            state, conf = R.make_state(cfg, seed=0), R.config_json(cfg)
        e = getattr(embeddings, cfg["cls"])(state=state, config=conf, tokenizer=tok, precision="f16", ctx=ctx)
        encoded = e.encode_texts(texts)
        lengths = [len(x) for x in encoded]
        groups = [tok.pad([encoded[i] for i in members], npad) for npad, members in e._groups(lengths, None)]
        rows = sum(ids.size for ids, _ in groups)
        whole = timed(lambda: e.embed_texts(texts), args.warmup, args.repeats, args.window)

        def cold():      # the tokenizer remembers the ids of ASCII words: forget them before every call
            tok._word_ids.clear()
            return e.embed_texts(texts)

        cold_cache = timed(cold, args.warmup, args.repeats, args.window)
        device = timed(lambda: [e.text_model.embed_ids_host(ids, lens) for ids, lens in groups], args.warmup, args.repeats, args.window)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for ids, lens in groups:
            e.text_model.embed_ids_host(ids, lens)
        prof = {k: round(v["total_ms"], 3) for k, v in ctx.profile_read().items() if v["launches"] and v["id"] not in IGEMM_TILE_SLOTS}
        ctx.profile_enable(False)
        emb = e.embed_texts(texts[:64])
        result[leg][name] = {
            "texts": len(texts),
            "dim_heads_depth_ffn": [cfg["dim"], cfg["heads"], cfg["depth"], cfg["ffn"]], "position": cfg["position"], "mlp": cfg["mlp"],
            "tokens": [min(lengths), max(lengths)], "calls": len(groups), "rows_per_text_by_call": [int(ids.shape[1]) for ids, _ in groups],
            "token_rows": int(rows), "tokens_total": int(sum(lengths)),
            "embed_texts": {"texts_per_s": round(len(texts) / whole[0], 1), "ms": round(whole[0] * 1e3, 3),
                            "ms_min_max": [round(whole[1] * 1e3, 3), round(whole[2] * 1e3, 3)], "calls_per_window": whole[3]},
            "embed_texts_word_cache_cleared": {"texts_per_s": round(len(texts) / cold_cache[0], 1), "ms": round(cold_cache[0] * 1e3, 3),
                                               "ms_min_max": [round(cold_cache[1] * 1e3, 3), round(cold_cache[2] * 1e3, 3)]},
            "encoder_calls_alone": {"texts_per_s": round(len(texts) / device[0], 1), "ms": round(device[0] * 1e3, 3),
                                    "ms_min_max": [round(device[1] * 1e3, 3), round(device[2] * 1e3, 3)],
                                    "gemm_tflops": round(rows * gflop_per_row(cfg) / device[0] / 1e3, 2)},
            "device_ms_by_kernel_family": prof, "device_ms_total": round(sum(prof.values()), 3),
            "attn_share": round(prof.get("attn_short", 0.0) / max(sum(prof.values()), 1e-9), 4),
            "finite": bool(np.isfinite(emb).all()), "largest_entry": round(float(np.abs(emb).max()), 3)}
        e.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
