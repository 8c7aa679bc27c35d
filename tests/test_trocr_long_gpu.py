"""TrOCR beam searches at the lengths the product runs (max_len_b = 200 by default; up to 640 keys of history), against the oracle
(oracle/trocr_torch.py) with the trace walk and certificate of oracle/trocr_trace.py.  ``make_trocr_sharp_state`` gives a decoder
with margins; ``min_len`` and ``end_fraction`` are chosen so that every hypothesis lives well past 64 steps and the lines end at
different lengths — the self-attention history crosses the f16 short-history kernel's 64-key limit, and in the second case the
256-key limit of the generic (1, 256) kernel, inside one search.

    case   decoder widths        max_len_b  max_positions  beam  lengths (oracle)        reaches
    A      (512, 2, 8, 2048)     200        256            3     91 .. 175               f16: fast kernel -> generic at 65 keys
    B      (256, 2, 4, 1024)     300        320            4     157 .. 293              generic (1, 256) -> (4, 640) at 257 keys
    base   trocr-base, 3 crops   200        512            3     (default configuration) the production configuration
    forced A, min_len = max_len  200        256            3     201 (every line)        finalisation at step == max_len, beam 3

fp32: no line diverges from the oracle in the walk, tokens equal, score within 2e-3.  f16: every divergence is a proven near-tie,
every certified line is token-equal, and every line is token-equal.  The last bar stands in for "at least half the lines are
certified": over 100 .. 300 steps the oracle's own searches finalise near-tied hypotheses (leads of a few 0.01 nats), so few lines
carry the certificate even at fp32 error (1 of 4 / 1 of 4 / 1 of 3 / 0 of 3), while f16 returned the oracle's tokens on all 14.
Measured on MI355X: candidate score error fp32 <= 1.2e-3 (no line diverged), f16 <= 0.29 before the first (explained) divergence;
final score |d| fp32 <= 1.4e-6, f16 <= 2.1e-3.  With MARIE_TEST_REPORT_DIR set, the numbers are written to trocr_long.json
there."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENC = (256, 2, 4)
VOCAB = 509
SHARP = dict(top_logit=45.0, fam_gain=12.0, img_gain=1.0, end_gain=6.0)
# name: (decoder widths, max_len_b, max_positions, beam, min_len, end_fraction, crops)
CASES = {
    "A": ((512, 2, 8, 2048), 200, 256, 3, 70, 0.01, 4),
    "B": ((256, 2, 4, 1024), 300, 320, 4, 150, 0.005, 4),
    "forced": ((512, 2, 8, 2048), 200, 256, 3, 200, 0.01, 3),
}
REPORT = {}


def _report(key, val):
    REPORT[key] = val
    d = os.environ.get("MARIE_TEST_REPORT_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "trocr_long.json"), "w") as f:
            json.dump(REPORT, f, indent=1, default=float)


@pytest.fixture(scope="module")
def ctx():
    import torch

    from marie_icr_amd._lib import Context

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    c = Context(0)
    yield c
    c.close()


def _cfg(ctx, enc, dec, vocab, max_positions, max_len_b, beam, min_len):
    from marie_icr_amd.trocr import default_config

    cfg = default_config(ctx.lib, "base")
    cfg.enc_dim, cfg.enc_depth, cfg.enc_heads = enc
    cfg.dec_dim, cfg.dec_layers, cfg.dec_heads, cfg.dec_ffn = dec
    cfg.vocab, cfg.max_positions, cfg.max_len_b, cfg.beam, cfg.min_len = vocab, max_positions, max_len_b, beam, min_len
    return cfg


_ORACLE = {}


def _case(ctx, name):
    """(state, cfg, crops, oracle hypotheses, oracle trace): the oracle runs once per case and module"""
    from marie_icr_amd.weights import make_image_u8, make_trocr_sharp_state
    from oracle.trocr_torch import TorchTrocrOracle

    if name not in _ORACLE:
        if name == "base":
            st = make_trocr_sharp_state(0, end_fraction=0.02, **SHARP)
            crops = make_image_u8(41, 3, 384, 384)
            from marie_icr_amd.trocr import default_config

            cfg = default_config(ctx.lib, "base")         # the default configuration, untouched but for min_len
            cfg.min_len = 70
            o = TorchTrocrOracle(st, 12, 16, beam=3, max_len_b=200, min_len=70)
        else:
            dec, mlb, mp, beam, min_len, ef, n = CASES[name]
            st = make_trocr_sharp_state(1, enc=ENC, dec=dec, vocab=VOCAB, max_positions=mp, end_fraction=ef, **SHARP)
            crops = make_image_u8(23, n, 384, 384)
            cfg = _cfg(ctx, ENC, dec, VOCAB, mp, mlb, beam, min_len)
            o = TorchTrocrOracle(st, ENC[2], dec[2], beam=beam, max_len_b=mlb, min_len=min_len)
        ref, otr = o.generate(crops, want_trace=True)
        _ORACLE[name] = (st, cfg, crops, ref, otr)
    return _ORACLE[name]


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("name", ["A", "B", "base", "forced"])
def test_long_search_matches_the_oracle(ctx, name, precision):
    from marie_icr_amd._lib import PREC_F16, PREC_F32
    from marie_icr_amd.trocr import TrocrModel
    from oracle import trocr_trace as tt

    st, cfg, crops, ref, otr = _case(ctx, name)
    prec = PREC_F32 if precision == "f32" else PREC_F16
    m = TrocrModel(ctx, st, cfg, prec)
    got, gtr = m.generate_trace_host(crops)
    again = m.generate_host(crops)                        # the product entry point returns what the traced one does
    m.close()
    for (a, sa), (b, sb) in zip(got, again):
        np.testing.assert_array_equal(a, b)
        assert sa == sb
    ML = m.max_len
    lens = [len(r[0]) for r in ref]
    # the searches really are long
    assert min(lens) > 64, lens
    if name == "B":
        assert max(lens) > 256, lens
    if name == "forced":
        assert all(n == ML + 1 for n in lens), (lens, ML)
        for t, _ in got:
            assert len(t) == ML + 1 and int(t[-1]) == cfg.eos and cfg.eos not in [int(v) for v in t[:-1]]
    else:
        assert len(set(lens)) >= 3, lens
    w = tt.walk(otr, gtr)
    equal = [bool(len(g[0]) == len(r[0]) and np.array_equal(g[0], r[0])) for g, r in zip(got, ref)]
    med = float(np.median([x["eps"] for x in w]))
    cert = tt.certificate(otr, ref, otr["finalized"], eos=cfg.eos, eps=[max(x["eps"], med) for x in w], factor=10.0)
    held = [c["holds"] for c in cert]
    rep = {"max_len": ML, "oracle_lengths": lens, "gpu_lengths": [len(g[0]) for g in got], "steps": int(gtr["scores"].shape[0]),
           "max_score_error": max(x["eps"] for x in w), "never_diverged": int(sum(x["diverged_at"] is None for x in w)),
           "tokens_equal": int(sum(equal)), "certified": int(sum(held)),
           "max_final_score_diff": max([abs(g[1] - r[1]) for g, r, e in zip(got, ref, equal) if e] or [0.0])}
    _report(f"{name}_{precision}", rep)
    for i, (x, e, c, (gt, gs), (rt, rs)) in enumerate(zip(w, equal, cert, got, ref)):
        assert x["explained"], (name, precision, i, x["diverged_at"], x["eps"])      # every divergence is a proven near-tie
        if x["diverged_at"] is None:
            assert e, (name, precision, i)
        if prec == PREC_F32:
            assert x["diverged_at"] is None and e and abs(gs - rs) <= 2e-3, (name, i, x["diverged_at"], gs, rs)
        elif c["holds"]:
            assert e, (name, i, c, x["eps"])
    if prec == PREC_F16:
        assert all(equal), rep


def test_two_entry_points_agree_at_max_len_200(ctx):
    """The batched path (recognize_pages_begin / add / finish) at max_len 200 returns what recognize_from_fragments returns on the
    same fragments — once in one search, once split because the pending crops exceed the effective decode batch."""
    from marie_icr_amd.fragments import FragmentList
    from marie_icr_amd.trocr import TrOcrProcessor

    st, cfg, *_ = _case(ctx, "A")
    rng = np.random.default_rng(29)
    frags = [rng.integers(0, 256, size=(int(h), int(w), 3)).astype(np.uint8)
             for h, w in ((40, 130), (25, 300), (60, 61), (33, 512), (48, 200))]
    for precision in ("f32", "f16"):
        p = TrOcrProcessor(state=st, config=cfg, precision=precision, ctx=ctx)
        ref = p.recognize_from_fragments(FragmentList(list(frags)))
        assert min(len(r["text"].split()) for r in ref) > 64
        page = np.zeros((64, 64, 3), np.uint8)
        for budget in (None, p.model.lib.mhip_trocr_workspace_bytes(p.model.h, 2) * 9 // 8):
            p.decode_budget_bytes = budget
            n = p.effective_decode_batch()
            assert n >= len(frags) if budget is None else n == 2                  # one search; three searches of <= 2 crops
            p.recognize_pages_begin(3)
            for b in (frags[:2], frags[2:3], frags[3:]):
                p.recognize_pages_add([(page, [[0, 0, 1, 1]] * len(b), FragmentList(list(b)), [1] * len(b))])
            out = p.recognize_pages_finish()
            got = [(w["text"], w["confidence"]) for res, _ in out for w in sorted(res["words"], key=lambda w: w["id"])]
            assert got == [(r["text"], round(r["confidence"], 3)) for r in ref], (precision, budget)


def test_decode_batch_fits_the_memory_budget_at_the_default_max_len(ctx):
    """trocr-base, the default configuration (max_len 200): the search the batched path runs fits a quarter of the device's memory
    including mhip_ensure_workspace's 1/8 headroom, and the bench's search shape (2560 crops, max_len_b 15) is still one search."""
    from marie_icr_amd._lib import PREC_F16
    from marie_icr_amd.trocr import TrocrModel, TrOcrProcessor, default_config

    budget = ctx.device_info()["hbm_bytes"] // 4
    cfg = default_config(ctx.lib, "base")
    assert cfg.max_len_b == 200 and cfg.max_positions == 512
    p = TrOcrProcessor(trocr_model=TrocrModel(ctx, None, cfg, PREC_F16), ctx=ctx)
    n = p.effective_decode_batch()
    p.recognize_pages_begin(0)
    assert p._decode_limit == n
    ws = lambda k: p.model.lib.mhip_trocr_workspace_bytes(p.model.h, k)
    assert 1 <= n < p.decode_batch and ws(n) * 9 // 8 <= budget < ws(n + 1) * 9 // 8, (n, ws(n), budget)
    _report("decode_batch_base_max_len_200", {"crops": n, "workspace_bytes": ws(n), "budget": budget})
    p.model.close()
    cfg.max_len_b = 15
    pb = TrOcrProcessor(trocr_model=TrocrModel(ctx, None, cfg, PREC_F16), ctx=ctx)
    nb = pb.effective_decode_batch()
    _report("decode_batch_base_max_len_15", {"crops": nb})
    assert nb >= 2560, nb
    pb.model.close()


def test_create_rejects_a_history_longer_than_decode_attention_runs(ctx):
    from marie_icr_amd._lib import PREC_F16, MarieHipError
    from marie_icr_amd.trocr import TrocrModel, default_config

    cfg = default_config(ctx.lib, "base")
    cfg.max_positions, cfg.max_len_b = 1024, 700
    with pytest.raises(MarieHipError, match="decode attention runs at most 640"):
        TrocrModel(ctx, None, cfg, PREC_F16)
    cfg.max_len_b = 639                                   # 640 keys at the last step: the limit itself
    m = TrocrModel(ctx, None, cfg, PREC_F16)
    assert m.max_len == 639
    m.close()
    # min_len above max_len = min(max_len_b, max_positions - 1): the generator asserts it (generator.py:63); accepted, eos would stay
    # masked at the forced last step and every line come back empty with score -inf
    for max_positions, max_len_b, min_len in ((512, 200, 201), (100, 200, 100)):
        cfg = default_config(ctx.lib, "base")
        cfg.max_positions, cfg.max_len_b, cfg.min_len = max_positions, max_len_b, min_len
        with pytest.raises(MarieHipError, match="min_len"):
            TrocrModel(ctx, None, cfg, PREC_F16)
    cfg = default_config(ctx.lib, "base")                 # min_len == max_len is the forced case of this module: accepted
    cfg.max_positions, cfg.max_len_b, cfg.min_len = 100, 200, 99
    m = TrocrModel(ctx, None, cfg, PREC_F16)
    assert m.max_len == 99
    m.close()
