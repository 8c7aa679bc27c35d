"""Times the CLIP vision tower (ViT-B/32, f16): python tools/bench_clip.py [--batches 1 16 64 256] [--repeats 7]

Seeded ViT-B/32 weights, seeded uint8 clips on the host.  Per batch size: `ClipVisionModel.embed_host` — clips up, the
encoder, the embeddings back, ending in a stream synchronise — warmed up, then `--repeats` timed windows of at least
`--window` seconds each; the figure is the median window's clips/s.  As a timing comparator only, the same tower through
`transformers` (CLIPVisionModelWithProjection, f16) on torch for the same card with the same host-to-host contract: uint8
clips up, normalise, forward, embeddings back.

Per-kernel share: run one batch size under the profiler, then summarise its statistics file:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_clip.py --profile-run 64
    python tools/bench_clip.py --stats-csv OUT/.../*kernel_stats.csv
The text tower (ViT-B/32 text geometry, f16): python tools/bench_clip.py --text [--batches 1 256 1024]
Per batch size, three-word texts over the synthetic vocabulary of tests/cliptext_ref.py, timed as `embed_texts` runs them —
the host tokeniser, then `ClipTextModel.embed_ids_host`: ids up, the tower, the embeddings back, ending in a stream
synchronise — and the tower call alone; then 256 texts of the full context (77 tokens in 80 rows).
Prints one JSON line.  Nothing is asserted on these numbers; this is not bench.py.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GFLOP_PER_CLIP = 4.4      # 12 layers x (4 D^2 + 2 D F) x 50 tokens + the patch projection, 2 FLOP per MAC


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


def short_name(name: str) -> str:
    """a kernel's name as the trace gives it (mangled or demangled) -> function name and template arguments"""
    m = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z_0-9]+?kernel)(I.*?E)?Ev", name)
    if m:
        return m.group(1) + ("<" + m.group(2)[1:-1] + ">" if m.group(2) else "")
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return name.split("(")[0][:70]


def summarise_stats(path: str) -> dict:
    """rocprofv3's kernel_stats.csv -> {kernel name (shortened): share of the summed kernel time}"""
    rows = list(csv.DictReader(open(path)))
    ns = lambda r: float(r["TotalDurationNs"]) if r.get("TotalDurationNs") else float(r["Calls"]) * float(r["AverageNs"])
    total = sum(ns(r) for r in rows)
    out = {}
    for r in sorted(rows, key=lambda r: -ns(r)):
        out[short_name(r["Name"])] = {"calls": int(r["Calls"]), "share": round(ns(r) / total, 4),
                                            "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    return out


def torch_comparator(state, cfg, device):
    """the same weights in transformers' CLIPVisionModelWithProjection, f16, on `device`: uint8 clips (host) -> embeddings (host)"""
    import torch
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    import clip_ref as R

    hf = CLIPVisionConfig(hidden_size=cfg["dim"], intermediate_size=cfg["ffn"], num_hidden_layers=cfg["depth"],
                          num_attention_heads=cfg["heads"], image_size=cfg["image_size"], patch_size=cfg["patch"],
                          projection_dim=cfg["proj_dim"], hidden_act="quick_gelu")
    model = CLIPVisionModelWithProjection(hf)
    model.load_state_dict(R.to_transformers(state), strict=False)
    model = model.half().eval().to(device)
    mean = torch.tensor(R.CLIP_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(R.CLIP_STD, device=device).view(1, 3, 1, 1)

    def run(clips: np.ndarray) -> np.ndarray:
        with torch.inference_mode():
            x = torch.from_numpy(clips).to(device).permute(0, 3, 1, 2).float() / 255
            return model(pixel_values=((x - mean) / std).half()).image_embeds.float().cpu().numpy()

    return run


def bench_text(args):
    """the text tower at ViT-B/32 text geometry: three-word texts per batch size, and 256 texts of the full context"""
    import tempfile

    import cliptext_ref as T
    from marie_icr_amd import embeddings
    from marie_icr_amd._lib import PREC_F16, Context
    from marie_icr_amd.clip_tokenizer import ClipTokenizer

    ctx = Context(0)
    with tempfile.TemporaryDirectory() as d:
        T.make_vocab(d)
        tok = ClipTokenizer.from_dir(d)
    tensors, c = embeddings.load_clip_text_state(T.make_state(T.VIT_B32_TEXT, seed=0))
    model = embeddings.ClipTextModel(ctx, tensors, c, PREC_F16)
    words = ("the", "invoice", "total")
    three = lambda i: " ".join(words[(i // 3 ** j) % 3] for j in range(3))
    cases = [(f"{B} three-word texts", [three(i) for i in range(B)]) for B in (args.batches or [1, 256, 1024])]
    cases.append(("256 texts of 77 tokens", [" ".join(words[(i + j) % 3] for j in range(75)) for i in range(256)]))
    result = {"model": "ViT-B/32 text tower", "precision": "f16", "device": ctx.device_info(), "cases": {}}
    for name, texts in cases:
        ids, eot = tok.encode_batch(texts)
        whole = timed(lambda: model.embed_ids_host(*tok.encode_batch(texts)), args.warmup, args.repeats, args.window)
        tower = timed(lambda: model.embed_ids_host(ids, eot), args.warmup, args.repeats, args.window)
        result["cases"][name] = {"rows_per_text": int(ids.shape[1]), "ms_per_call": round(whole[0] * 1e3, 3),
                                 "ms_min_max": [round(whole[1] * 1e3, 3), round(whole[2] * 1e3, 3)],
                                 "tower_ms_per_call": round(tower[0] * 1e3, 3),
                                 "tower_ms_min_max": [round(tower[1] * 1e3, 3), round(tower[2] * 1e3, 3)],
                                 "texts_per_s": round(len(texts) / whole[0], 1), "calls_per_window": whole[3],
                                 "workspace_mb": round(model.workspace_bytes(len(texts), ids.shape[1]) / 2**20, 1)}
    model.close()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", action="store_true", help="time the text tower instead")
    ap.add_argument("--batches", type=int, nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3, help="least seconds of one timed window")
    ap.add_argument("--no-comparator", action="store_true")
    ap.add_argument("--profile-run", type=int, default=0, metavar="B", help="only run 20 warm calls at batch B (under a profiler)")
    ap.add_argument("--stats-csv", default=None, help="summarise a rocprofv3 kernel_stats.csv and exit")
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps({"kernel_share": summarise_stats(args.stats_csv)}))
        return
    if args.text:
        return bench_text(args)
    args.batches = args.batches or [1, 16, 64, 256]

    import clip_ref as R
    from marie_icr_amd import embeddings
    from marie_icr_amd._lib import PREC_F16, Context

    ctx = Context(0)
    cfg = R.VIT_B32
    state = R.make_state(cfg, *R.GAINS["vit_b32"], seed=0)
    tensors, c = embeddings.load_clip_vision_state(state)
    model = embeddings.ClipVisionModel(ctx, tensors, c, PREC_F16)
    rng = np.random.default_rng(0)
    clips = rng.integers(0, 256, (max(args.batches + [args.profile_run]), 224, 224, 3)).astype(np.uint8)
    if args.profile_run:
        for _ in range(20):
            model.embed_host(clips[:args.profile_run])
        return

    result = {"model": "ViT-B/32", "precision": "f16", "device": ctx.device_info(), "gflop_per_clip": GFLOP_PER_CLIP, "hip": {}}
    for B in args.batches:
        med, lo, hi, calls = timed(lambda: model.embed_host(clips[:B]), args.warmup, args.repeats, args.window)
        result["hip"][B] = {"clips_per_s": round(B / med, 1), "ms_per_call": round(med * 1e3, 3),
                            "ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)], "calls_per_window": calls,
                            "tflops": round(B * GFLOP_PER_CLIP / med / 1e3, 2), "workspace_mb": round(model.workspace_bytes(B) / 2**20, 1)}
    if not args.no_comparator:
        import torch

        run = torch_comparator(state, cfg, f"cuda:{ctx.device_id}")
        diff = float(np.abs(run(clips[:8]) - model.embed_host(clips[:8])).max())
        result["comparator"] = {"what": "transformers CLIPVisionModelWithProjection f16 on torch", "torch": torch.__version__,
                                "max_abs_diff_to_hip_f16": round(diff, 5)}
        for B in args.batches:
            med, lo, hi, calls = timed(lambda: run(clips[:B]), args.warmup, args.repeats, args.window)
            result["comparator"][B] = {"clips_per_s": round(B / med, 1), "ms_per_call": round(med * 1e3, 3),
                                       "ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)]}
    model.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
