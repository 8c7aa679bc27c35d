"""Times VQ-NNF template matching on one page: python tools/bench_template_matching.py [--templates 8] [--steps 5]

One seeded 2550 x 3300 page against `--templates` templates at the reference's default window (384 x 128, overlap 0.2: 275
slices): the batched device call alone (`VQNNFTemplateMatcher.match_windows`: page upload, nearest-code assignment, heat maps
and `--max-objects` peak rounds over the whole slice x template grid, peaks back), template state cached.  Prints one JSON
line: slices/s, (slice, template) pairs/s, the per-call times and, from a profiled call, the device time per kernel.
Nothing is asserted on these numbers; this is not bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_page(seed: int, h: int, w: int) -> np.ndarray:
    """white page with seeded dark strokes and a few tinted regions (uint8 HxWx3)"""
    rng = np.random.default_rng(seed)
    page = np.full((h, w, 3), 255, np.uint8)
    for _ in range(h * w // 900):
        y, x = int(rng.integers(0, h - 4)), int(rng.integers(0, w - 24))
        page[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(4, 24))] = rng.integers(0, 120, 3)
    for _ in range(12):
        y, x = int(rng.integers(0, h - 200)), int(rng.integers(0, w - 300))
        page[y:y + 200, x:x + 300] = np.minimum(page[y:y + 200, x:x + 300], rng.integers(180, 250, 3).astype(np.uint8))
    return page


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-objects", type=int, default=1)
    ap.add_argument("--page", type=int, nargs=2, default=(3300, 2550), metavar=("H", "W"))
    ap.add_argument("--window", type=int, nargs=2, default=(384, 128), metavar=("H", "W"))
    args = ap.parse_args()

    from marie_icr_amd import template_matching as tmx
    from marie_icr_amd._lib import Context

    ctx = Context(0)
    page = make_page(1, *args.page)
    wh, ww = args.window
    rng = np.random.default_rng(2)
    boxes = [(int(rng.integers(0, 2500 - 160)), int(rng.integers(0, 3200 - 60)), int(rng.integers(60, 120)),
              int(rng.integers(24, 48))) for _ in range(args.templates)]
    frames, tboxes = tmx.BaseTemplateMatcher.extract_windows(page, boxes, (wh, ww))
    windows = tmx.slice_image(page.shape[0], page.shape[1], wh, ww)
    m = tmx.VQNNFTemplateMatcher("bench", ctx=ctx)
    t0 = time.perf_counter()
    for f, b in zip(frames, tboxes):
        m.template_state(f, b)
    ctx.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    times = []
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        m.match_windows(page, windows, frames, tboxes, args.max_objects)
        if i >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    ctx.profile_reset()
    m.match_windows(page, windows, frames, tboxes, args.max_objects)
    ctx.synchronize()
    prof = {k: round(v["total_ms"], 3) for k, v in ctx.profile_read().items() if k.startswith("vq_") and v["launches"]}
    ctx.profile_enable(False)
    med = float(np.median(times))
    print(json.dumps({"page": list(page.shape[:2]), "window": [wh, ww], "slices": len(windows), "templates": args.templates,
                      "max_objects": args.max_objects, "template_build_ms_total": round(build_ms, 2),
                      "kmeans_iterations": [t.iterations for t in m.cached_features.values()],
                      "call_ms_median": round(med, 3), "call_ms_min": round(min(times), 3), "call_ms_max": round(max(times), 3),
                      "slices_per_s": round(len(windows) / med * 1e3, 1),
                      "pairs_per_s": round(len(windows) * args.templates / med * 1e3, 1), "kernel_ms": prof}))
    m.close()
    ctx.close()


if __name__ == "__main__":
    main()
