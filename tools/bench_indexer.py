"""First throughput measurement of the document indexer's model call: windows/s and pages/s in f16 through
``mhip_layoutlmv3_tag`` for pages of 1, 2 and 4 windows, with the windows of a page sharing its resize and patch projection and,
for comparison, with the page copied per window (the identity window -> page map: what the reference hands its model).

Method: seeded base-size weights (13 labels, dense head) and 1100 x 850 pages whose sub-token counts fill 1, 2 and 4 windows;
``--pages`` pages per call (already on the device; token ids / boxes on the host as the indexer passes them); per shape W
warm-up calls, then K timed calls, wall clock around each call (the call returns after the stream drained); the median call and
the spread (min / max) are printed.  Prints one JSON line.

    python tools/bench_indexer.py [--steps 10] [--warmup 3] [--pages 8]
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
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pages", type=int, default=8)
    args = ap.parse_args()

    import torch

    import indexer_ref as IR
    from marie_icr_amd._lib import PREC_F16, Context
    from marie_icr_amd.document_classifier import ByteLevelBPE
    from marie_icr_amd.document_indexer import normalize_bbox
    from marie_icr_amd.layoutlmv3 import LayoutLMv3Model, default_config, pack_pages
    from marie_icr_amd.weights import make_layoutlmv3_token_state, make_page_bgr, write_synthetic_bpe

    ctx = Context(0)
    model = LayoutLMv3Model(ctx, make_layoutlmv3_token_state(0, 13), default_config(ctx.lib, num_labels=13), PREC_F16)
    with tempfile.TemporaryDirectory() as d:
        write_synthetic_bpe(d, seed=1)
        tok = ByteLevelBPE(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"))
    h, w = 1100, 850
    result = {"tool": "bench_indexer", "precision": "f16", "device": ctx.device_info()["arch"], "page": [h, w],
              "pages_per_call": args.pages, "windows_per_page": {}}
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for n_win, n_sub in ((1, 500), (2, 880), (4, 1640)):
        pages, wp, enc = [], [], []
        for i in range(args.pages):
            pages.append(make_page_bgr(800 + i, h, w))
            words, boxes = IR.make_words(900 + i, n_sub, tok, w, h, exact=True)
            e = tok.encode_windows(words, [normalize_bbox(b, (w, h)) for b in boxes])
            assert e[0].shape[0] == n_win
            enc.append(e)
            wp += [i] * n_win
        ids, bbox, mask = (np.concatenate([e[j] for e in enc]) for j in range(3))
        entry = {"text_tokens_mean": float(mask.sum(1).mean())}
        for mode in ("shared", "copied"):
            imgs = pages if mode == "shared" else [pages[p] for p in wp]
            win_page = np.asarray(wp if mode == "shared" else range(len(wp)), np.int32)
            packed, descs = pack_pages(imgs)
            d_in = torch.from_numpy(packed).cuda()
            torch.cuda.synchronize()
            times = []
            for it in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                model.tag_device(d_in.data_ptr(), descs, len(imgs), win_page, ids, bbox, mask)
                if it >= args.warmup:
                    times.append(time.perf_counter() - t0)
            med = float(np.median(times))
            entry[mode] = {"windows_per_s": len(wp) / med, "pages_per_s": args.pages / med, "ms_per_call_median": med * 1e3,
                           "ms_per_call_min": min(times) * 1e3, "ms_per_call_max": max(times) * 1e3}
        entry["sharing_speedup"] = entry["copied"]["ms_per_call_median"] / entry["shared"]["ms_per_call_median"]
        result["windows_per_page"][str(n_win)] = entry
    model.close()
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
