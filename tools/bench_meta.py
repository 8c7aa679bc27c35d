"""Times MetaTemplateMatcher's edit-distance step on one page: python tools/bench_meta.py [--words 2000] [--templates 50]

A seeded word-level page (words of 1 .. 12 letters over A-Z and digits, some of them copies of template words with an edit) and
seeded templates of 1 .. 6 words.  Timed, host arrays in to host arrays out:
  * `text_layout`, the host side of a `predict` (the page as one string of alphabet ids);
  * `lev_ngrams_host`: ids up, the kernel (csrc/lev_ngrams.hip), distances and lengths back, ending in a stream synchronise —
    warmed up, then `--repeats` windows of at least `--window` seconds, the figure is the median window's ms per call; the
    kernel alone from the library's profiler (hipEvents around the launch);
  * the same distances by the two-row Python DP of tests/meta_ref.py, one pair at a time as the reference loops, on a seeded
    subsample of `--dp-pairs` pairs, scaled to all pairs of the page (pairs differ in length: the scaling is by DP cells).
The kernel's result is compared with the DP on the subsample first.  Prints one JSON line.  Nothing is asserted on these
numbers; this is not bench.py.
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

LETTERS = list("ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789")


def timed(fn, warmup: int, repeats: int, window: float):
    """median seconds per call over `repeats` windows of >= `window` seconds"""
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


def make_case(n_words: int, n_templates: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    word = lambda: "".join(rng.choice(LETTERS, int(rng.integers(1, 13))))
    texts = [" ".join(word() for _ in range(int(rng.integers(1, 7)))) for _ in range(n_templates)]
    words = [word() for _ in range(n_words)]
    for t in texts[::2]:                                  # half of the templates occur on the page, one of them with an edit
        at = int(rng.integers(0, n_words - 8))
        parts = t.lower().split(" ")
        words[at:at + len(parts)] = parts
        words[at] = words[at][:-1] + "x"
    lines = (np.arange(n_words) // 12).tolist()
    return words, texts, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=2000)
    ap.add_argument("--templates", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3, help="least seconds of one timed window")
    ap.add_argument("--dp-pairs", type=int, default=1500, help="pairs of the Python DP subsample")
    args = ap.parse_args()

    import meta_ref as R
    from marie_icr_amd import template_matching as tmx
    from marie_icr_amd._lib import Context

    ctx = Context(0)
    words, texts, lines = make_case(args.words, args.templates)
    patterns = [t.strip().upper() for t in texts]
    g = [len(t.split(" ")) for t in texts]
    layout = tmx.text_layout(words, patterns)
    result = {"device": ctx.device_info(), "words": len(words), "templates": len(texts), "page_code_points": len(layout.page_ids),
              "alphabet": layout.alphabet, "pattern_code_points": [int(np.diff(layout.pattern_off).min()),
                                                                  int(np.diff(layout.pattern_off).max())]}
    for name, ln in (("no_lines", None), ("lines", lines)):
        dist, length = tmx.lev_ngrams_host(ctx, layout, g, ln)
        t_idx, k_idx, i_idx = np.nonzero(dist >= 0)
        m = np.diff(layout.pattern_off)[t_idx]
        cells = float((length[t_idx, k_idx, i_idx].astype(np.int64) * m).sum())
        med, lo, hi, calls = timed(lambda: tmx.lev_ngrams_host(ctx, layout, g, ln), args.warmup, args.repeats, args.window)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(20):
            tmx.lev_ngrams_host(ctx, layout, g, ln)
        prof = ctx.profile_read()["lev_ngrams"]
        ctx.profile_enable(False)
        # the Python DP on a subsample, the reference's way: build the n-gram string, then the distance
        pick = np.random.default_rng(1).choice(len(t_idx), min(args.dp_pairs, len(t_idx)), replace=False)
        sub_cells, wrong = 0.0, 0
        t0 = time.perf_counter()
        for p in pick:
            t, k, i = int(t_idx[p]), int(k_idx[p]), int(i_idx[p])
            text = R.ngram_text(words, i, g[t] - 1 + k)
            wrong += R.dp_distance(text, patterns[t]) != dist[t, k, i] or len(text) != length[t, k, i]
            sub_cells += len(text) * len(patterns[t])
        dp_s = time.perf_counter() - t0
        result[name] = {"pairs": int(len(t_idx)), "dp_cells": cells, "call_ms": round(med * 1e3, 3),
                        "call_ms_min_max": [round(lo * 1e3, 3), round(hi * 1e3, 3)], "calls_per_window": calls,
                        "kernel_ms": round(prof["total_ms"] / max(prof["launches"], 1), 4),
                        "launches_per_call": prof["launches"] / 20,
                        "python_dp_subsample": {"pairs": int(len(pick)), "seconds": round(dp_s, 3), "wrong": int(wrong)},
                        "python_dp_page_seconds_scaled": round(dp_s * cells / max(sub_cells, 1.0), 2)}
    lay = timed(lambda: tmx.text_layout(words, patterns), 1, 3, 0.1)
    result["text_layout_ms"] = round(lay[0] * 1e3, 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
