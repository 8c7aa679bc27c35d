"""LayoutReader reading order on the MI355X (marie_icr_amd/csrc/layoutreader_api.hip, layoutreader_ops.hip) against
tests/layoutreader_ref.py, the float64 restatement that tests/test_layoutreader_cpu.py pins to the model itself through
tests/golden/layoutreader.npz.

Bars:
  * fp32: 1e-3 absolute on O(1) quantities (attention outputs, stream taps) and on the scores; the golden's smallest top-2 margin
    is 0.074, so every one of the 128 decisions must be the golden's;
  * f16: E_ref = max |f16-rounded restatement - float64| is computed here on the CPU for the same inputs, and
    max |kernel - float64| <= 2 E_ref: the factor allows about one more rounding per stage where the kernel's rounding points and
    accumulation order differ from the emulation.  The model is compared step by step with the golden decisions forced, so that
    one flipped decision cannot cascade; the arg-max is asserted at every step whose golden margin is >= 10 x the measured score
    error, and the steps set aside are at most a quarter (tests/test_layoutreader_cpu.py proves the cap for E_ref);
  * a page's decisions and scores do not depend on the call it is part of: bitwise, in both precisions.
Every test prints its figures before it asserts.
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layoutreader_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layoutreader.npz")
F32, F16 = 1, 0
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    for key in [k for k in _cache if k[0] == "model"]:
        _cache.pop(key).close()
    c.close()


@pytest.fixture(scope="module")
def lr():
    from marie_icr_amd import layoutreader

    return layoutreader


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


def _model(ctx, lr, golden, precision, name="golden", state=None):
    key = ("model", name, precision)
    if key not in _cache:
        tensors, cfg = lr.load_layoutreader_state(golden["state"] if state is None else state, R.config_json(golden["cfg"]))
        _cache[key] = lr.LayoutReaderModel(ctx, tensors, cfg, precision)
    return _cache[key]


def _reference(golden, forced, f16):
    """the restatement on the golden pages, computed once and left unchanged"""
    key = ("ref", forced, f16)
    if key not in _cache:
        out = R.run_pages(golden["state"], golden["cfg"], golden["pages"], forced=golden["decisions"] if forced else None, f16=f16)
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _run(ctx, lr, golden, precision, forced):
    """the four golden pages in one debug call, once per (precision, forced)"""
    key = ("run", precision, forced)
    if key not in _cache:
        _cache[key] = _model(ctx, lr, golden, precision).debug_host(golden["pages"], forced=golden["decisions"] if forced else None)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- decode attention alone
HEADS, D = 2, 128


def _attn_inputs(pages, nq, cache_rows, tgt_base, seed):
    """pages: [(source length, targets so far)].  Cache rows past a page's lengths hold NaN: they must not be read"""
    rng = np.random.default_rng(seed)
    P = len(pages)
    q = rng.standard_normal((P, nq, D)) * (R.LOG2E / 8.0)
    k = rng.standard_normal((P, nq, D))
    v = rng.standard_normal((P, nq, D)) + np.linspace(-1, 1, D)
    kc = rng.standard_normal((P, cache_rows, D)) + 0.3 * np.linspace(-1, 1, cache_rows)[None, :, None]
    vc = rng.standard_normal((P, cache_rows, D)) + np.linspace(-1, 1, D)
    for p, (ns, nt) in enumerate(pages):
        for c in (kc, vc):
            c[p, ns:tgt_base] = np.nan
            c[p, tgt_base + nt:] = np.nan
    src = np.array([ns for ns, _ in pages], np.int32)
    tgt = np.repeat(np.array([nt for _, nt in pages], np.int32), nq).reshape(P, nq)
    return [np.ascontiguousarray(a, np.float32) for a in (q, k, v, kc, vc)] + [src, tgt]


def _attn_ref(q, k, v, kc, vc, src, tgt, tgt_base):
    q, k, v, kc, vc = (np.asarray(a, np.float64) for a in (q, k, v, kc, vc))
    out = np.zeros_like(q)
    for p in range(q.shape[0]):
        for i in range(q.shape[1]):
            sel = lambda c, own: np.concatenate([c[p, :src[p]], c[p, tgt_base:tgt_base + tgt[p, i]], own[p, :i + 1]])  # noqa: E731
            out[p, i] = R.attend(q[p, i], sel(kc, k), sel(vc, v), HEADS)
    return out


# (source length, targets so far): the shortest source with no and one target; the golden's source with the key count around 64
# (34 + 29 + own = 64); the production maximum, 513 + 510 + own = 1024 keys (1025 for the second of two rows), beside a shorter
# page in the same launch
ATTN_LAUNCHES = {"S34": (66, 34, [(3, 0), (3, 1), (34, 29), (34, 30), (34, 31)]), "S513": (1024, 513, [(513, 510), (200, 77)])}


# first MI355X run: f32 1.4e-7 .. 4.8e-7; f16 max |kernel - fp64| 4.55e-4 (S513, one row), 5.24e-4 (S513, two rows), 8.10e-4 (S34,
# one row), 9.40e-4 (S34, two rows), each equal to E_ref of its case to the four digits printed
@pytest.mark.parametrize("launch", list(ATTN_LAUNCHES))
@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_decode_attention_kernel(ctx, lr, precision, nq, launch):
    cache_rows, tgt_base, pages = ATTN_LAUNCHES[launch]
    q, k, v, kc, vc, src, tgt = _attn_inputs(pages, nq, cache_rows, tgt_base, 5)
    want = _attn_ref(q, k, v, kc, vc, src, tgt, tgt_base)
    got = lr.decode_attention_host(ctx, precision, q, k, v, kc, vc, src, tgt, HEADS, tgt_base)
    err = float(np.abs(got - want).max())
    assert np.isfinite(got).all(), "a cache row past a page's lengths was read"
    assert 0.5 <= np.abs(want).max() <= 8
    if precision == F32:
        print(f"lr_decode_attn f32 {launch} nq {nq}: max |d| {err:.3e}")
        assert err <= 1e-3
    else:
        emu = R.r16(_attn_ref(R.r16(q), R.r16(k), R.r16(v), R.r16(kc), R.r16(vc), src, tgt, tgt_base))
        e_ref = float(np.abs(emu - want).max())
        print(f"lr_decode_attn f16 {launch} nq {nq}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        assert err <= 2 * e_ref
    # a page does not depend on the pages it is launched with: bitwise
    p = len(pages) - 1
    alone = lr.decode_attention_host(ctx, precision, q[p:], k[p:], v[p:], kc[p:], vc[p:], src[p:], tgt[p:], HEADS, tgt_base)
    assert np.array_equal(alone[0], got[p])
    if nq == 2:
        # the first row does not see the second: launched as the only row it gives the same bits
        one = lr.decode_attention_host(ctx, precision, q[:, :1], k[:, :1], v[:, :1], kc, vc, src, tgt[:, :1], HEADS, tgt_base)
        assert np.array_equal(one[:, 0], got[:, 0])


# ---------------------------------------------------------------------------------------------------- embedding and pointer select
def test_embedding_and_source_taps_fp32(ctx, lr, golden):
    run, ref = _run(ctx, lr, golden, F32, False), _reference(golden, False, False)
    e_emb = float(np.abs(run["emb"] - golden["emb"]).max())
    e_last = float(np.abs(run["last"] - ref["last"]).max())
    print(f"fp32 source pass: embedded rows max |d| {e_emb:.3e} (vs the model), last layer max |d| {e_last:.3e} (vs the restatement)")
    assert e_emb <= 1e-3 and e_last <= 1e-3
    # rows past [SEP] of the last-layer tap are not computed
    for p, page in enumerate(golden["pages"]):
        assert not run["last"][p, len(page) + 2:].any()


def test_pointer_select_takes_the_lowest_index_on_ties(ctx, lr, golden):
    """One position row for every position and a constant bias make source rows with equal boxes equal rows of E: the five words
    (one box), and [CLS] with the pads (box 0).  Their scores are then equal bit for bit, every step's maximum is shared unless
    [SEP] holds it, and the decision must be the lowest index of the class: 0 ([CLS], never a pad) or 1 (never words 2 .. 5)."""
    state = dict(golden["state"])
    pos = state["bert.embeddings.position_embeddings.weight"]
    state["bert.embeddings.position_embeddings.weight"] = np.repeat(pos[:1], len(pos), 0)
    state["cls.predictions.bias"] = np.full_like(state["cls.predictions.bias"], 0.25)
    n = 5
    page = np.array([[100, 200, 180, 230]] * n, np.int32)
    out = _model(ctx, lr, golden, F32, "ties", state).debug_host([page])
    s, d = out["scores"][0], out["decisions"][0]
    assert np.array_equal(s[:, 1:n + 1], np.repeat(s[:, 1:2], n, 1)) and np.array_equal(s[:, n + 2:], np.repeat(s[:, :1], s.shape[1] - n - 2, 1))
    tied = int(sum((row == row.max()).sum() > 1 for row in s))
    print(f"pointer select: {tied} of {len(s)} steps have a shared maximum; decisions {sorted(set(d.tolist()))}")
    assert tied >= 1
    assert np.array_equal(d, s.argmax(-1))          # numpy's arg-max is the first of the maxima
    assert set(d.tolist()) <= {0, 1, n + 1}


# ---------------------------------------------------------------------------------------------------- the model
# first MI355X run: fp32 128 of 128 decisions, scores max |d| 2.11e-5 (embedded rows 4.7e-7, last source layer 1.6e-6);
# f16 forced: scores max |d| 0.0239 against E_ref 0.0238 on scores within +-37, 7 of 128 steps (5.5 %) set aside, 128 of 128
# decisions equal; f16 free-running: 128 of 128, page 2 the only one with no step set aside
def test_fp32_free_running_equals_the_golden(ctx, lr, golden):
    run = _run(ctx, lr, golden, F32, False)
    err = float(np.abs(run["scores"] - golden["scores"]).max())
    same = int((run["decisions"] == golden["decisions"]).sum())
    print(f"fp32 free-running: {same} of {golden['decisions'].size} decisions equal, scores max |d| {err:.3e}")
    assert np.array_equal(run["decisions"], golden["decisions"])
    assert err <= 1e-3
    assert np.array_equal(_model(ctx, lr, golden, F32).order_host(golden["pages"]), run["decisions"])


def _f16_forced(ctx, lr, golden):
    run, ref16 = _run(ctx, lr, golden, F16, True), _reference(golden, True, True)
    e_ref = float(np.abs(ref16["scores"] - golden["scores"]).max())
    err = np.abs(run["scores"] - golden["scores"]).max(-1)           # (pages, T)
    aside = R.margins(golden["scores"]) < 10 * float(err.max())
    return run, e_ref, err, aside


def test_f16_forced_scores_and_decisions(ctx, lr, golden):
    run, e_ref, err, aside = _f16_forced(ctx, lr, golden)
    print(f"f16 forced: scores max |d| {float(err.max()):.4f}, E_ref {e_ref:.4f} (scores within +-{np.abs(golden['scores']).max():.0f}); "
          f"{int(aside.sum())} of {aside.size} steps ({aside.mean():.1%}) have a golden margin below 10 x the error; "
          f"{int((run['decisions'] == golden['decisions']).sum())} decisions equal")
    assert float(err.max()) <= 2 * e_ref
    assert aside.mean() <= 0.25
    assert np.array_equal(run["decisions"][~aside], golden["decisions"][~aside])


def test_f16_free_running(ctx, lr, golden):
    _, _, _, aside = _f16_forced(ctx, lr, golden)
    run = _run(ctx, lr, golden, F16, False)
    same = run["decisions"] == golden["decisions"]
    print(f"f16 free-running: {int(same.sum())} of {same.size} decisions equal the golden's; pages with no step set aside: "
          f"{[p for p in range(len(aside)) if not aside[p].any()]}")
    for p in range(len(aside)):
        if not aside[p].any():
            assert same[p].all(), f"page {p}"


@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_a_page_does_not_depend_on_its_batch(ctx, lr, golden, precision):
    run = _run(ctx, lr, golden, precision, False)
    m = _model(ctx, lr, golden, precision)
    for p, page in enumerate(golden["pages"]):
        alone = m.debug_host([page])
        assert np.array_equal(alone["decisions"][0], run["decisions"][p]), f"page {p}"
        assert np.array_equal(alone["scores"][0], run["scores"][p]), f"page {p}"
        assert np.array_equal(alone["emb"][0], run["emb"][p]) and np.array_equal(alone["last"][0], run["last"][p])


def test_text_layout_reconstruct_end_to_end(ctx, lr, golden):
    layout = lr.TextLayout(state=golden["state"], config=R.config_json(golden["cfg"]), precision="f32", ctx=ctx)
    try:
        assert layout.max_len == 32
        batch = layout.forward_batch(golden["pages"])
        for p, page in enumerate(golden["pages"]):
            words, boxes = [f"w{i}" for i in range(len(page))], page.tolist()
            idx = (golden["decisions"][p].astype(np.int64) - 1).tolist()
            assert layout.forward(words, boxes) == idx and batch[p] == idx
            assert layout(words, boxes) == lr.reorder(words, boxes, idx)
        words, boxes = [str(i) for i in range(33)], [[0, 0, 1, 1]] * 33
        out = layout.reconstruct(words, boxes)
        assert out[0] is words and out[1] is boxes
        with pytest.raises(ValueError):
            layout.forward(words, boxes)
        with pytest.raises(ValueError):
            layout.forward(["a"], [[0, 0, 1001, 1]])
    finally:
        layout.close()


# ---------------------------------------------------------------------------------------------------- production shape
PROD = dict(dim=768, heads=12, depth=12, ffn=3072, max_source=513, max_position=1024, max_2d=1024, type_vocab=2, source_type=0,
            target_type=1, eps=1e-5)


# first MI355X run: 1 page 494 ms a call, 8 pages 603 ms a call; workspace 49 / 317 MiB (DESIGN.md §3 `layoutreader` has the profile)
def test_production_shape_runs(ctx, lr):
    """dim 768, 12 layers, S = 513, all 511 steps, f16: one page of 200 words, and 8 pages in one call"""
    S, T = PROD["max_source"], PROD["max_source"] - 2
    tensors, cfg = lr.load_layoutreader_state(R.make_state(PROD, 3), R.config_json(PROD))
    m = lr.LayoutReaderModel(ctx, tensors, cfg, F16)
    try:
        pages = R.make_pages(PROD, 3, words=(200, 1, 64, 130, 257, 400, 480, 511))
        one = m.debug_host(pages[:1])
        t0 = time.perf_counter()
        d1 = m.order_host(pages[:1])
        t1 = time.perf_counter()
        d8 = m.order_host(pages)
        t2 = time.perf_counter()
        eight = m.debug_host(pages)
        print(f"production shape, f16, {T} steps: 1 page {1e3 * (t1 - t0):.0f} ms a call, 8 pages {1e3 * (t2 - t1):.0f} ms a call; "
              f"workspace {m.workspace_bytes(1) / 2**20:.0f} / {m.workspace_bytes(8) / 2**20:.0f} MiB; "
              f"{len(set(one['decisions'][0].tolist()))} distinct decisions on the page of 200 words")
        for out in (one, eight):
            assert np.isfinite(out["scores"]).all()
            assert out["decisions"].min() >= 0 and out["decisions"].max() <= S - 1
        assert np.array_equal(d1, one["decisions"]) and np.array_equal(d8, eight["decisions"])
        assert np.array_equal(eight["decisions"][0], one["decisions"][0]) and np.array_equal(eight["scores"][0], one["scores"][0])
    finally:
        m.close()
