"""BASELINE configs[2] at its REAL size, both precisions, against the oracle — through the C ABI.

One seeded 2550 x 3300 page -> DiT-base (resize to 1035 x 800, 3301 tokens, 12 layers, FPN, RPN, ROI heads) and four of its
line crops -> TrOCR-base (DeiT 12 x 768, decoder 12 x 1024, vocabulary 50 265, beam 3).  The reference's path:
marie/detectron/detector.py:83-147, marie/boxes/dit/ulim_dit_box_processor.py:441-499,
marie/models/unilm/trocr/generator.py:127-362.  The oracle's detectron2 / fairseq stages are parity-unpinned (oracle headers).

Bars (written next to each assertion):
  fp32  FPN maps and RPN-head outputs within 2e-3; discrete stages replayed on identical inputs give identical sets (boxes
        within 2e-3 px, scores exact / 1e-6); end to end every box the interval analysis (oracle/dit_trace.py) marks KEPT has
        a partner at IoU >= 0.999 (boxes of a few pixels, whose IoU moves by 0.3 % under a 0.004 px shift: every coordinate
        within the measured error, < 0.01 px) and every extra / missing box is a proven near-tie; TrOCR tokens exact, score
        within 1e-3.  Measured (profiles/r03/b_fullsize_parity.json): 911 / 911 boxes, 876 KEPT and all matched, max |d coordinate| 0.004 px.
  f16   (the bench dtype) maps within 0.5 % of range; the same interval analysis with f16's measured error: every KEPT box
        matched, every f16 box a KEPT or UNSTABLE candidate, matched pairs within the predicted coordinate error; box-set match
        fractions reported and bounded; TrOCR: every divergence of the beam search a proven near-tie (40 lines), and on the
        decoder with margins every certified line string-exact (80 lines).
Numbers are written to gpurun_out/fullsize_parity.json when that directory exists."""
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAGE_H, PAGE_W, LINES = 3300, 2550, 40
REPORT = {}


def _report(key, val, report=REPORT, name="fullsize_parity.json"):
    """also the writer of the other parity reports (tests/test_gemm_fold_gpu.py): `report` into the file `name`"""
    report[key] = val
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, name), "w") as f:
            json.dump(report, f, indent=1, default=float)


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def page():
    from marie_icr_amd.weights import make_page_bgr

    return make_page_bgr(999, PAGE_H, PAGE_W, n_lines=LINES)


@pytest.fixture(scope="module")
def dit_case(page):
    import torch

    from marie_icr_amd.weights import make_dit_state
    from oracle.dit_torch import TorchDitOracle

    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    st = make_dit_state(0, "base")
    o = TorchDitOracle(st)
    t0 = time.perf_counter()
    boxes, scores, stages = o.detect(page, want_stages=True)
    _report("dit_oracle_seconds", time.perf_counter() - t0)
    return st, o, boxes, scores, stages


def _match(ref, got, bar):
    from oracle.dit_trace import pair_iou

    iou = pair_iou(ref, got)
    return float((iou.max(axis=1) >= bar).mean()) if len(ref) and len(got) else 0.0


def test_dit_base_fp32_full_page(ctx, page, dit_case):
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.dit import DitModel, det_final, roi_align, rpn_proposals
    from oracle import dit_torch as dt
    from oracle import dit_trace as tr

    st, o, rboxes, rscores, stages = dit_case
    m = DitModel(ctx, st, model="base", precision=PREC_F32)
    out = m.debug_host(page)
    m.close()
    nh, nw = stages["resized_hw"]
    assert out["resized_hw"] == (nh, nw) == (1035, 800)
    sizes, strides = out["sizes"], (4, 8, 16, 32, 64)

    # ---- continuous stages: fp32 within 2e-3 (north_star: logits within 1e-3 fp32; FPN sums four taps) ----
    e_fpn = [float(np.abs(f - r).max()) for f, r in zip(out["fpn"], stages["fpn"])]
    e_rpn = [float(np.abs(g - r).max()) for g, r in zip(out["rpn_heads"], stages["rpn_heads"])]
    assert max(e_fpn) <= 2e-3, e_fpn
    assert max(e_rpn) <= 2e-3, e_rpn

    # ---- discrete stages on IDENTICAL inputs, both directions: identical sets ----
    # (a) the GPU's RPN selection / FastRCNN inference on the oracle's tensors == the oracle's outputs
    gb, gs = rpn_proposals(ctx, stages["rpn_heads"], sizes, strides, (nh, nw))
    assert len(gb) == len(stages["proposals"])
    np.testing.assert_array_equal(gs, stages["proposal_scores"])
    assert np.abs(gb - stages["proposals"]).max() <= 1e-3
    nhwc = [np.ascontiguousarray(f) for f in stages["fpn"][:4]]
    pooled = roi_align(ctx, nhwc, stages["proposals"])
    assert np.abs(pooled - stages["pooled"]).max() <= 2e-5
    fb, fs = det_final(ctx, stages["head"], stages["proposals"], (nh, nw), (PAGE_H, PAGE_W))
    assert len(fb) == len(rboxes)
    assert np.abs(fs - rscores).max() <= 1e-6
    assert np.abs(fb - rboxes).max() <= 2e-3          # px on a 2550 x 3300 page: IoU >= 0.9999 for any box over 40 px^2
    assert _match(rboxes, fb, 0.999) == 1.0
    # (b) the oracle's discrete stages on the GPU run's own tensors == what the GPU run produced
    ob, os_ = dt.rpn_proposals(out["rpn_heads"], sizes, strides, (nh, nw), dt.cell_anchors())
    assert len(ob) == len(out["proposals"])
    np.testing.assert_array_equal(os_, out["proposal_scores"])
    assert np.abs(ob - out["proposals"]).max() <= 1e-3
    ofb, ofs = dt.fast_rcnn_inference(out["head"], out["proposals"], (nh, nw), (PAGE_H, PAGE_W))
    assert len(ofb) == len(out["boxes"])
    assert np.abs(ofs - out["scores"]).max() <= 1e-6
    assert np.abs(ofb - out["boxes"]).max() <= 2e-3

    # ---- end to end: every miss is a near-tie (oracle/dit_trace.py) ----
    ex = tr.explain_end_to_end(o, stages, out, (PAGE_H, PAGE_W))
    chk_p, chk = ex["proposals_check"], ex["boxes_check"]
    assert ex["eps_logit"] <= 2e-3 and ex["eps_prob"] <= 2e-3 and ex["eps_page_px"] <= 1e-2, ex    # a detection moves < 0.01 px
    assert ex["proposals_on_both"] >= 0.9 * len(out["proposals"])
    assert not chk_p["missing_kept"] and not chk_p["foreign"], chk_p
    rep = {"fpn_max_abs_err": e_fpn, "rpn_head_max_abs_err": e_rpn, "oracle_boxes": len(rboxes), "gpu_boxes": len(out["boxes"]),
           "oracle_proposals": len(stages["proposals"]), "gpu_proposals": len(out["proposals"]), **ex,
           "matched_iou_0.999": _match(rboxes, out["boxes"], 0.999), "matched_iou_0.99": _match(rboxes, out["boxes"], 0.99)}
    _report("dit_base_fp32", rep)
    # the bar: IoU >= 0.999 for every box whose existence does not hang on a near-tie; nothing unexplained on either side
    assert not chk["missing_kept"], rep
    assert not chk["foreign"], rep
    assert chk["kept_matched"] == chk["kept"] and chk["kept"] >= 0.5 * len(rboxes), rep
    assert len(rboxes) > 100


def test_dit_base_f16_full_page(ctx, page, dit_case):
    """The bench dtype: f16 operands, fp32 accumulation / residual stream."""
    from marie_icr_amd._lib import PREC_F16
    from marie_icr_amd.dit import DitModel
    from oracle import dit_torch as dt
    from oracle import dit_trace as tr

    st, o, rboxes, rscores, stages = dit_case
    m = DitModel(ctx, st, model="base", precision=PREC_F16)
    out = m.debug_host(page)
    again = m.detect_host(page[None])[0]
    m.close()
    np.testing.assert_array_equal(again[0], out["boxes"])          # the debug path and the product path agree
    rel = []
    for f, r in zip(out["fpn"], stages["fpn"]):
        rng_ = float(np.abs(r).max())
        rel.append(float(np.abs(f - r).max()) / rng_)
        assert np.abs(f - r).max() <= 0.005 * rng_, (np.abs(f - r).max(), rng_)      # 0.5 % of range (measured 0.09 - 0.12 %)
    # the discrete stages are precision-independent: replay the oracle's on the f16 run's own tensors
    nh, nw = stages["resized_hw"]
    ob, os_ = dt.rpn_proposals(out["rpn_heads"], out["sizes"], (4, 8, 16, 32, 64), (nh, nw), dt.cell_anchors())
    assert len(ob) == len(out["proposals"])
    np.testing.assert_array_equal(os_, out["proposal_scores"])
    assert np.abs(ob - out["proposals"]).max() <= 1e-3
    ofb, ofs = dt.fast_rcnn_inference(out["head"], out["proposals"], (nh, nw), (PAGE_H, PAGE_W))
    assert len(ofb) == len(out["boxes"]) and np.abs(ofb - out["boxes"]).max() <= 2e-3
    e_rpn = [float(np.abs(g - r).max()) for g, r in zip(out["rpn_heads"], stages["rpn_heads"])]
    rep = {"fpn_max_err_over_range": rel, "rpn_head_max_abs_err": e_rpn, "oracle_boxes": len(rboxes),
           "gpu_boxes": len(out["boxes"]), "matched_iou_0.999": _match(rboxes, out["boxes"], 0.999),
           "matched_iou_0.99": _match(rboxes, out["boxes"], 0.99), "matched_iou_0.9": _match(rboxes, out["boxes"], 0.9),
           "matched_iou_0.5": _match(rboxes, out["boxes"], 0.5)}
    # ---- the fp32 argument with f16's MEASURED error: interval analysis of the oracle's discrete stages (oracle/dit_trace.py)
    # eps = 1.5 x the error of this run's own RPN-head / box-head tensors.  Every candidate the oracle keeps under every
    # perturbation up to eps (KEPT) must be in the f16 run's output — at IoU >= 0.999 or every coordinate within the coordinate
    # error the measured head error predicts (eps_page_px) — and every box the f16 run returns must be a KEPT or UNSTABLE
    # candidate: every difference between the two box sets is a proven near-tie, nothing is unexplained on either side.
    ex = tr.explain_end_to_end(o, stages, out, (PAGE_H, PAGE_W))
    chk_p, chk = ex["proposals_check"], ex["boxes_check"]
    rep.update({k: v for k, v in ex.items()})
    _report("dit_base_f16", rep)
    assert not chk_p["missing_kept"] and not chk_p["foreign"], chk_p
    assert not chk["missing_kept"] and not chk["foreign"], chk
    assert chk["kept_matched"] == chk["kept"], chk
    # matched pairs: a box of the f16 run sits within the predicted coordinate error of the candidate it realises
    # (within 0.2 % of the box extent = IoU >= 0.999 territory, or within eps_page_px for the small boxes)
    assert chk["max_coord_dev_px_of_pairs_beyond_0.2pct"] <= ex["eps_page_px"] + 1e-6, (chk, ex["eps_page_px"])
    # random weights make every page position a candidate with near-equal scores, so f16 map noise re-orders many discrete
    # choices (the KEPT count says how many of the oracle's decisions have a margin above this run's error); the f16 run still
    # finds the same structures: count within 10 %, overlap >= 0.5 for 80 %
    assert abs(len(out["boxes"]) - len(rboxes)) <= 0.1 * len(rboxes), rep
    assert rep["matched_iou_0.5"] >= 0.8, rep


@pytest.fixture(scope="module")
def trocr_case(page):
    import torch

    from marie_icr_amd.weights import make_trocr_state, page_line_boxes
    from oracle.trocr_torch import TorchTrocrOracle, preprocess_fragments

    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    enc, dec, vocab, maxpos = (768, 12, 12), (1024, 12, 16, 4096), 50265, 512
    st = make_trocr_state(0, enc, dec, vocab, maxpos)
    lines = page_line_boxes(PAGE_H, PAGE_W, LINES)
    frags = [page[y:y + h + 1, x:x + w + 1] for x, y, w, h in lines[[0, 7, 19, 33]].tolist()]
    o = TorchTrocrOracle(st, enc[2], dec[2], beam=3, max_len_b=15)
    crops = preprocess_fragments(frags)
    t0 = time.perf_counter()
    ref, step0 = o.generate(crops, want_step0=True)
    _report("trocr_oracle_seconds", time.perf_counter() - t0)
    return st, frags, crops, o, ref, step0


def _trocr_cfg(ctx):
    from marie_icr_amd.trocr import default_config

    cfg = default_config(ctx.lib, "base")
    assert (cfg.enc_dim, cfg.enc_depth, cfg.dec_dim, cfg.dec_layers, cfg.vocab, cfg.beam) == (768, 12, 1024, 12, 50265, 3)
    cfg.max_len_b = 15
    return cfg


def test_trocr_base_fp32_real_dimensions(ctx, trocr_case):
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.trocr import TrocrModel

    st, frags, crops, o, ref, step0 = trocr_case
    m = TrocrModel(ctx, st, _trocr_cfg(ctx), PREC_F32)
    got, enc, lg = m.generate_host(crops, want_taps=True)
    m.close()
    e_enc = float(np.abs(enc - o.encode(crops).numpy()).max())
    e_lg = float(np.abs(lg - step0).max())
    _report("trocr_base_fp32", {"encoder_max_abs_err": e_enc, "step0_logits_max_abs_err": e_lg,
                                "tokens": [[int(t) for t in g[0]] for g in got], "scores": [g[1] for g in got],
                                "oracle_scores": [r[1] for r in ref]})
    assert e_enc <= 1e-3 and e_lg <= 2e-3, (e_enc, e_lg)            # fp32 logits bar (12 + 12 layers, 50 265 columns)
    for (gt, gs), (rt, rs) in zip(got, ref):
        np.testing.assert_array_equal(gt, rt)                      # string-exact for the same decode rule
        assert abs(gs - rs) <= 1e-3


def test_trocr_base_f16_real_dimensions(ctx, trocr_case):
    """The bench dtype through the fragment entry point the engine and bench.py use (ragged vocabulary 50 265 -> pitch 50 272
    logits epilogue, 577-token encoder, 12 + 12 layers)."""
    import torch

    from marie_icr_amd._lib import PREC_F16
    from marie_icr_amd.crnn import pack_fragments
    from marie_icr_amd.trocr import TrocrModel

    st, frags, crops, o, ref, step0 = trocr_case
    m = TrocrModel(ctx, st, _trocr_cfg(ctx), PREC_F16)
    packed, descs = pack_fragments(frags)
    d_in = torch.from_numpy(packed).cuda()
    got = m.generate_fragments(d_in.data_ptr(), descs, len(frags), swap_rb=True)
    got_host, enc, lg = m.generate_host(crops, want_taps=True)
    m.close()
    for (a, sa), (b, sb) in zip(got, got_host):                    # the fused resize equals Pillow's crops
        np.testing.assert_array_equal(a, b)
        assert abs(sa - sb) <= 1e-5
    e_lg = float(np.abs(lg - step0).max())
    equal = [bool(len(g[0]) == len(r[0]) and np.array_equal(g[0], r[0])) for g, r in zip(got, ref)]
    own = o.score_tokens(crops, [g[0] for g in got])               # the oracle's score of the f16 run's hypotheses
    gaps = [float(r[1] - s) for r, s in zip(ref, own)]
    _report("trocr_base_f16", {"step0_logits_max_abs_err": e_lg, "step0_logit_range": float(np.abs(step0).max()),
                               "hypotheses_equal": equal, "oracle_best_minus_oracle_score_of_f16_hypothesis": gaps,
                               "f16_scores": [g[1] for g in got], "oracle_scores": [r[1] for r in ref]})
    assert e_lg <= 0.02 * float(np.abs(step0).max()) + 0.05
    for eq, gap, (gt, gs), (rt, rs) in zip(equal, gaps, got, ref):
        # equal tokens, or a hypothesis the ORACLE itself scores within 0.005 nats/token of its best (a near-tie: this seeded
        # model repeats a token and switches to another one at a step where the two are almost equally likely; measured gaps
        # 3e-4 and -8e-4 — the second one is a hypothesis the oracle scores HIGHER than what its own beam search returned)
        assert eq or gap <= 0.005, (gap, gt, rt)
        if eq:
            assert abs(gs - rs) <= 0.02
    assert sum(equal) >= len(equal) // 2


# ---- the beam search as a chain of decisions: all 40 lines of the page, f16 against the oracle, step by step --------------------
def _lines_of(pages_seeds):
    from marie_icr_amd.weights import make_page_bgr, page_line_boxes
    from oracle.trocr_torch import preprocess_fragments

    boxes = page_line_boxes(PAGE_H, PAGE_W, LINES)
    frags = []
    for seed in pages_seeds:
        pg = make_page_bgr(seed, PAGE_H, PAGE_W, n_lines=LINES)
        frags += [pg[y:y + h + 1, x:x + w + 1] for x, y, w, h in boxes.tolist()]
    return preprocess_fragments(frags)


def _walk_case(ctx, state, crops, precision):
    import torch

    from marie_icr_amd.trocr import TrocrModel
    from oracle import trocr_trace as tt
    from oracle.trocr_torch import TorchTrocrOracle

    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    o = TorchTrocrOracle(state, 12, 16, beam=3, max_len_b=15)
    ref, otr = o.generate(crops, want_trace=True)
    m = TrocrModel(ctx, state, _trocr_cfg(ctx), precision)
    got, gtr = m.generate_trace_host(crops)
    again = m.generate_host(crops)                       # the product entry point returns what the traced one does
    m.close()
    for (a, sa), (b, sb) in zip(got, again):
        np.testing.assert_array_equal(a, b)
        assert sa == sb
    return o, ref, otr, got, gtr, tt.walk(otr, gtr)


def test_trocr_base_f16_every_divergence_on_the_page_is_a_near_tie(ctx, trocr_case):
    """The 40 lines of the page through TrOCR-base, beam 3, f16, with the candidate list of every step read back
    (mhip_trocr_generate_trace_host) and walked beside the oracle's (oracle/trocr_trace.py).  While the two lists agree the
    score error of every candidate is measured; where they first differ, the oracle's own list must hold the candidates in
    question within 2 x 1.5 x that measured error of each other.  A line that never diverges returns the oracle's tokens.
    fp32 on the same lines: no line diverges at all.  (This seeded decoder has no margins — logits of random projections — so
    near-ties are frequent; the model with margins is the next test.)"""
    from marie_icr_amd._lib import PREC_F16, PREC_F32

    st = trocr_case[0]
    crops = _lines_of([999])
    assert len(crops) == LINES
    rep = {}
    for name, prec in (("f32", PREC_F32), ("f16", PREC_F16)):
        o, ref, otr, got, gtr, w = _walk_case(ctx, st, crops, prec)
        equal = [bool(len(g[0]) == len(r[0]) and np.array_equal(g[0], r[0])) for g, r in zip(got, ref)]
        never = [x["diverged_at"] is None for x in w]
        rep[name] = {"lines": len(crops), "tokens_equal": int(sum(equal)), "never_diverged": int(sum(never)),
                     "diverged_explained": int(sum((not n) and x["explained"] for n, x in zip(never, w))),
                     "diverged_unexplained": int(sum((not n) and (not x["explained"]) for n, x in zip(never, w))),
                     "max_score_error": max(x["eps"] for x in w),
                     "symbol_error_rate": _ser([list(map(int, r[0])) for r in ref], [list(map(int, g[0])) for g in got])}
        for i, (x, eq, (gt, gs), (rt, rs)) in enumerate(zip(w, equal, got, ref)):
            assert x["explained"], (name, i, x)                                  # every divergence is a proven near-tie
            if x["diverged_at"] is None:
                assert eq, (name, i)                                             # same decisions -> same string
                assert abs(gs - rs) <= (2e-3 if prec == PREC_F32 else 1.5 * x["eps"] + 1e-4)
        if prec == PREC_F32:
            assert all(never) and all(equal) and rep[name]["max_score_error"] <= 2e-3, rep[name]
    _report("trocr_base_page_walk", rep)
    assert rep["f16"]["tokens_equal"] >= LINES // 2, rep["f16"]


def _ser(refs, hyps):
    dist = total = 0
    for r, h in zip(refs, hyps):
        prev = list(range(len(h) + 1))
        for i, a in enumerate(r, 1):
            cur = [i]
            for j, b in enumerate(h, 1):
                cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a != b)))
            prev = cur
        dist += prev[-1]
        total += len(r)
    return dist / max(1, total)


def test_trocr_base_f16_model_with_margins_is_string_exact(ctx):
    """north_star: "string-exact for the same decode rule".  ``make_trocr_sharp_state`` is TrOCR-base with structure at the
    decoder's two ends (two designed successors per token, the winner decided by the previous token, the position and the
    image; marie_icr_amd/weights.py) so that the oracle's own search has margins.  80 lines (two seeded pages).  For every line whose
    oracle run carries the certificate of oracle/trocr_trace.py — best hypothesis = chain of top-1 candidates, every top-1 /
    top-2 gap of cumulative score >= 10 x the f16 score error MEASURED on that line's candidates, lead over the other finished
    hypotheses >= 10 x that error / length — the f16 run must return the same tokens; there must be at least 40 such lines; every other
    line is equal or diverges at a proven near-tie.  Sequences are not degenerate: no immediate repeats, several different
    strings, lines ending at different lengths."""
    from marie_icr_amd._lib import PREC_F16
    from marie_icr_amd.weights import make_trocr_sharp_state
    from oracle import trocr_trace as tt

    st = make_trocr_sharp_state(0, top_logit=45.0, fam_gain=12.0, img_gain=1.0, end_fraction=0.15, end_gain=6.0)
    crops = _lines_of([999, 998])
    o, ref, otr, got, gtr, w = _walk_case(ctx, st, crops, PREC_F16)
    eps = max(x["eps"] for x in w)
    # the error bound of a line: what the walk measured on that line's own candidates (every step of a line that never diverged),
    # never less than the median over the lines
    med = float(np.median([x["eps"] for x in w]))
    cert = tt.certificate(otr, ref, otr["finalized"], eos=2, eps=[max(x["eps"], med) for x in w], factor=10.0)
    equal = [bool(len(g[0]) == len(r[0]) and np.array_equal(g[0], r[0])) for g, r in zip(got, ref)]
    held = [c["holds"] for c in cert]
    strings = {tuple(int(v) for v in r[0]) for r in ref}
    rep = {"lines": len(crops), "measured_score_error": eps, "median_line_score_error": med, "certified_lines": int(sum(held)),
           "certified_and_equal": int(sum(h and e for h, e in zip(held, equal))), "tokens_equal": int(sum(equal)),
           "never_diverged": int(sum(x["diverged_at"] is None for x in w)), "distinct_strings": len(strings),
           "lengths": sorted({len(r[0]) for r in ref}), "min_certified_gap": min([c["min_gap"] for c in cert if c["holds"]] or [0.0]),
           "max_final_score_diff": max(abs(g[1] - r[1]) for g, r, e in zip(got, ref, equal) if e),
           "symbol_error_rate": _ser([list(map(int, r[0])) for r in ref], [list(map(int, g[0])) for g in got])}
    _report("trocr_base_f16_margin_model", rep)
    for i, (c, e, x) in enumerate(zip(cert, equal, w)):
        if c["holds"]:
            assert e, (i, c, x)                                  # margins >= 10 x the measured error: string-exact
        assert x["explained"], (i, x)
        if x["diverged_at"] is None:
            assert e, i
    assert sum(held) >= 40, rep
    assert sum(equal) >= 0.95 * len(crops), rep                  # measured: 80 of 80 lines token-equal
    assert len(strings) >= 3 and len(rep["lengths"]) >= 2, rep
    for r in ref:
        t = [int(v) for v in r[0]]
        assert all(a != b for a, b in zip(t, t[1:])), t        # no token repeated back to back
