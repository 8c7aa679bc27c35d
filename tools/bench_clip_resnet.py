"""Times CLIP's ModifiedResNet tower (RN50x4, f16 by default): python tools/bench_clip_resnet.py [--batches 1 8 32] [--repeats 7]

Seeded RN50x4 weights (tests/clip_resnet_ref.py), seeded uint8 clips on the host.  Per batch size: `ClipResNetModel.embed_host` —
clips up, the tower, the embeddings back, ending in a stream synchronise — warmed up, then `--repeats` timed windows of at
least `--window` seconds each; the figure is the median window's clips/s.  Then, in a pass of its own with the library's event
profiler on (it slows the host, so it is kept out of the timed windows), the device time per profile slot at the largest
batch: the share of conv_igemm in the summed kernel time.  The FLOPs of a clip are counted from the checkpoint's shapes (no
padding channels), 2 per multiply-add.
Prints one JSON line.  Nothing is asserted on these numbers; this is not bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def gflop_per_clip(cfg: dict) -> float:
    """the tower's multiply-adds from the shapes: the stem, every Bottleneck, the attention pool's projections"""
    import clip_resnet_ref as R

    w, S = cfg["width"], cfg["image_size"]
    mac = (S // 2) ** 2 * (27 * (w // 2) + 9 * (w // 2) * (w // 2) + 9 * (w // 2) * w)
    H = S // 4
    for _, cin, planes, stride, down in R.blocks(cfg):
        Ho = H // stride
        mac += H * H * (cin * planes + 9 * planes * planes) + Ho * Ho * planes * 4 * planes
        if down:
            mac += Ho * Ho * cin * 4 * planes
        H = Ho
    E, NT = 32 * w, R.n_tokens(cfg)
    mac += E * E + NT * 2 * E * E + 2 * NT * E + E * cfg["proj_dim"]
    return 2 * mac / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--precision", choices=["f16", "f32"], default="f16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds of one timed window")
    ap.add_argument("--profile-calls", type=int, default=10, help="calls of the profiled pass at the largest batch (0: none)")
    args = ap.parse_args()

    import clip_resnet_ref as R
    from marie_icr_amd import embeddings
    from marie_icr_amd._lib import PREC_F16, PREC_F32, Context

    ctx = Context(0)
    cfg = R.RN50X4
    tensors, c = embeddings.load_clip_resnet_state(R.make_state(cfg, R.GAINS["rn50x4"], seed=0))
    model = embeddings.ClipResNetModel(ctx, tensors, c, PREC_F16 if args.precision == "f16" else PREC_F32)
    rng = np.random.default_rng(0)
    S = cfg["image_size"]
    clips = rng.integers(0, 256, (max(args.batches), S, S, 3)).astype(np.uint8)
    gf = gflop_per_clip(cfg)
    result = {"model": "RN50x4", "precision": args.precision, "device": ctx.device_info(), "gflop_per_clip": round(gf, 2), "hip": {}}
    for B in args.batches:
        med, lo, hi, calls = timed(lambda: model.embed_host(clips[:B]), args.warmup, args.repeats, args.window)
        result["hip"][B] = {"clips_per_s": round(B / med, 1), "ms_per_call": round(med * 1e3, 3),
                            "ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)], "calls_per_window": calls,
                            "tflops_end_to_end": round(B * gf / med / 1e3, 2), "workspace_mb": round(model.workspace_bytes(B) / 2**20, 1)}
    if args.profile_calls:
        B = max(args.batches)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.profile_calls):
            model.embed_host(clips[:B])
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        # the tile slots are counted in conv_igemm as well: leave them out of the sum
        top = {k: v for k, v in prof.items() if v["launches"] and not k.startswith("conv_igemm<") and k != "conv3x3_patch"}
        total = sum(v["total_ms"] for v in top.values())
        result["profile"] = {"batch": B, "calls": args.profile_calls, "kernel_ms_per_call": round(total / args.profile_calls, 3),
                             "share": {k: round(v["total_ms"] / total, 4) for k, v in sorted(top.items(), key=lambda kv: -kv[1]["total_ms"])},
                             "launches_per_call": {k: v["launches"] // args.profile_calls for k, v in top.items()},
                             "conv_igemm_tflops": round(prof["conv_igemm"]["flops"] / max(prof["conv_igemm"]["total_ms"], 1e-9) / 1e9, 2),
                             "conv_igemm_tiles_ms": {k: round(v["total_ms"] / args.profile_calls, 3) for k, v in prof.items()
                                                     if k.startswith("conv_igemm<") and v["launches"]}}
    model.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
