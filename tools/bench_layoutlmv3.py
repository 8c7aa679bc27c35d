"""First throughput measurement of the LayoutLMv3 page classifier: pages/s at batch 16 and 64 in f16 through
``mhip_layoutlmv3_classify`` (pages already on the device, token ids / boxes on the host as the classifier passes them), and the
share of device time in the biased attention kernel.

Method: seeded base-size weights and pages (1100 x 850 frames, about 250 sub-tokens each); per batch size W warm-up calls, then K
timed calls, wall clock around each call (the call returns after the stream drained); the median call and the spread
(min / max) are printed.  The kernel shares come from a separate profiled pass (event pairs around every launch), not from the
timed one.  Prints one JSON line.

    python tools/bench_layoutlmv3.py [--steps 10] [--warmup 3] [--batches 16,64]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="16,64")
    args = ap.parse_args()

    import torch

    from marie_icr_amd._lib import PREC_F16, Context
    from marie_icr_amd.document_classifier import ByteLevelBPE, scale_bounding_box
    from marie_icr_amd.layoutlmv3 import LayoutLMv3Model, default_config, pack_pages
    from marie_icr_amd.renderer import get_words_and_boxes
    from marie_icr_amd.weights import make_layoutlmv3_state, make_ocr_result, make_page_bgr, write_synthetic_bpe

    ctx = Context(0)
    model = LayoutLMv3Model(ctx, make_layoutlmv3_state(0), default_config(ctx.lib, num_labels=7), PREC_F16)
    with tempfile.TemporaryDirectory() as d:
        write_synthetic_bpe(d, seed=1)
        tok = ByteLevelBPE(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"))
    h, w = 1100, 850
    result = {"tool": "bench_layoutlmv3", "precision": "f16", "device": ctx.device_info()["arch"], "page": [h, w], "batches": {}}
    for bs in [int(v) for v in args.batches.split(",")]:
        pages, enc = [], []
        for i in range(bs):
            pages.append(make_page_bgr(500 + i, h, w))
            words, boxes = get_words_and_boxes([make_ocr_result(600 + i, w, h, n_lines=12)], 0)
            enc.append(tok.encode_page(words, [scale_bounding_box(b, 1000 / w, 1000 / h) for b in boxes]))
        ids, bbox, mask = (np.stack([e[j] for e in enc]) for j in range(3))
        packed, descs = pack_pages(pages)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        d_in = torch.from_numpy(packed).cuda()
        torch.cuda.synchronize()
        times = []
        for it in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            model.classify_device(d_in.data_ptr(), descs, bs, ids, bbox, mask)
            if it >= args.warmup:
                times.append(time.perf_counter() - t0)
        ctx.profile_enable(True)
        ctx.profile_reset()
        model.classify_device(d_in.data_ptr(), descs, bs, ids, bbox, mask)
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        top = {k: v["total_ms"] for k, v in prof.items() if "<" not in k and v["total_ms"] > 0}      # tile variants are counted in conv_igemm
        total = sum(top.values())
        med = float(np.median(times))
        result["batches"][str(bs)] = {
            "pages_per_s": bs / med, "ms_per_call_median": med * 1e3, "ms_per_call_min": min(times) * 1e3,
            "ms_per_call_max": max(times) * 1e3, "text_tokens_mean": float(mask.sum(1).mean()),
            "attn_bias_share": top.get("attn_bias", 0.0) / total if total else None,
            "attn_bias_tflops": (prof["attn_bias"]["flops"] / (prof["attn_bias"]["total_ms"] * 1e-3) / 1e12) if prof["attn_bias"]["total_ms"] else None,
            "kernel_ms": {k: round(v, 3) for k, v in sorted(top.items(), key=lambda kv: -kv[1])}}
    model.close()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
