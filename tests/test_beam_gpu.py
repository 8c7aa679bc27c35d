"""Kernel-level tests of the TrOCR decoder's per-step beam search: beam_candidates_kernel<float | _Float16> and ancestry_kernel
(csrc/trocr_ops.hip), beam_init / beam_select / beam_best (csrc/beam_state.hip), alone through mhip_beam_candidates_host and
mhip_beam_search_host, against oracle/beam_ref.py: log_softmax + masks + stable order in fp64 on the logits as the device holds
them, and integer-exact restatements of the generator's bookkeeping.

The candidates kernel alone, oracle/beam_ref.GPU_CASES in both logit types (tests/test_oracle_beam.py proves on the CPU that in
every case adjacent scores are bit-equal ties or 4 x score_bound apart, that an emulation of the kernel passes and that ten seeded
kernel bugs do not).  Per case: the (token, beam) lists equal the reference's exactly; every score within score_bound, -inf exactly
-inf, none NaN; scores non-increasing; one dec_ops launch; the 16 guard elements behind each list still 0xff.

The search in logits mode (vocabulary 24, max_len 6, beams 1 .. 4, 65 crops and 1): step by step the device's lists against the
reference on the device's own cum, then everything beam_select / ancestry / beam_best wrote against the restatement fed the
device's own lists, then the free-running fp64 search.  One batch that ends early runs again with 2 extra steps: same bits.
The search in candidates mode: the hand-written lists of beam_ref.list_cases().  Refusals: both entries, nothing written.

score_bound supposes 1 ulp for the hardware exp2 and for logf (neither is documented to us).  Measured on MI355X, the largest
max err / bound over the cases of a group, f16 | fp32 logits — every ratio stayed under 1, the worst is 0.41:
    candidates, by placement   spread 0.166 | 0.146   one_chunk 0.128 | 0.122   one_wave 0.098 | 0.123   per_wave 0.110 | 0.131
                               col0 0.099 | 0.124   last_col 0.103 | 0.105   rows_gt0 0.083 | 0.120   same_col 0.102 | 0.105
                               vocabulary 50265 (beams 3, 4; 2 crops) 0.053 | 0.055
    ties                       constant_row 0.136 | 0.151   identical_rows 0.074 | 0.065
    masks                      on_pad 0.156 | 0.168   on_eos 0.098 | 0.119   step0_nan 0.113 | 0.090   step0_decoys 0.110 | 0.111
    non-finite                 nan 0.083 | 0.115   nan_alone 0.069 | 0.065   posinf 0.083 | 0.115   neginf_row 0.083 | 0.115
                               neginf_runs 0.114 | 0.110   cum_neginf 0.083 | 0.115   magnitude 0.136 | 0.115
    search, every step         bsz 65: beam 1 .. 4  0.385 0.391 0.354 0.372 | 0.361 0.371 0.411 0.399
                               bsz 1:  beam 1 .. 4  0.123 0.152 0.184 0.128 | 0.145 0.189 0.178 0.268
The CPU emulation (libm's exp2) peaks at 0.156 | 0.168 on the same candidates cases.
magnitude: +-65504 in f16; in fp32 the last row of every crop holds +1e30 and -1e30 beside zeros, with a finite cum — its winner must
score cum exactly (score_bound takes each rounding as at most its smaller operand, so lse = 1e30 + logf(1) costs nothing), the zeros tie
at -1e30 — and row 0 carries a -1e30 among finite logits.

What the 295 tests of this module do to wrong kernels, on scratch builds (not committed):
    beam_candidates_kernel as it was before this work (a chunk of -inf skipped although a NaN hides in it): the 8 nan_alone cases
        fail — the row's other logits keep finite scores where log_softmax makes the whole row NaN — and nothing else;
    the higher flat index wins a tie (key low word = flat index): 57 fail — every constant_row, step == max_len and step > max_len
        case, identical_rows at beams 2 .. 4, the -inf lists of the non-finite cases, the zeros that tie at -1e30 beside the fp32
        +1e30 (beam 1), all 16 scripted searches;
    a lane offers only K - 1 of its shortlist to the wave rounds, and beam_best takes the last hypothesis on a tie: 70 fail — all
        8 one_chunk cases, the small vocabularies (2 * beam, 8, 9) whose list one lane holds, 14 of the 16 searches; the beam_best
        half fails ignore-inf-ties-never alone.

The ratios are written to beam_errors.json beside the other parity reports (test_fullsize_gpu._report)."""
import ctypes as C

import numpy as np
import pytest

from oracle import beam_ref as R
from test_fullsize_gpu import _report

pytestmark = pytest.mark.gpu

ERRORS = {}
PARAMS = R.case_params()
vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
NULL = C.c_void_p(0)


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _launches(ctx, fn):
    """fn() with the profile counters on -> (rc, launches of dec_ops kernels)"""
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        rc = fn()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    return rc, prof.get("dec_ops", {}).get("launches", 0)


def _candidates(ctx, case):
    """one mhip_beam_candidates_host call -> cand_scores, cand_tokens, cand_beams [bsz][2 * beam]; asserts one launch, whole guards"""
    from marie_icr_amd._lib import check

    n = case["bsz"] * 2 * case["beam"]
    cs, ct, cb = np.zeros(n + R.GUARD, np.float32), np.zeros(n + R.GUARD, np.int32), np.zeros(n + R.GUARD, np.int32)
    L, cum = np.ascontiguousarray(case["logits"]), np.ascontiguousarray(case["cum"], np.float32)
    assert L.dtype == (np.float16 if case["f16"] else np.float32) and L.shape == (case["bsz"] * case["beam"], case["ld"])
    rc, launches = _launches(ctx, lambda: ctx.lib.mhip_beam_candidates_host(
        ctx.h, int(case["f16"]), vp(L), vp(cum), case["step"], case["max_len"], case["min_len"], case["pad"], case["eos"],
        case["vocab"], case["ld"], case["beam"], case["bsz"], vp(cs), vp(ct), vp(cb)))
    check(ctx.h, rc, "mhip_beam_candidates_host")
    assert launches == 1, launches
    for a in (cs, ct, cb):
        assert (a[n:].view(np.uint32) == 0xFFFFFFFF).all(), "the guard elements behind a list were written"
    shape = (case["bsz"], 2 * case["beam"])
    return cs[:n].reshape(shape), ct[:n].reshape(shape), cb[:n].reshape(shape)


def _check_lists(tag, ref, cs, ct, cb, crops=None):
    """the assertions on one launch's lists against candidates() -> max err / bound"""
    worst = 0.0
    for s, r in enumerate(ref):
        if crops is not None and s not in crops:
            continue
        K = len(r["cand_tokens"])
        print(f"{tag} crop {s}: dev {cs[s].tolist()} tokens {ct[s].tolist()} beams {cb[s].tolist()} | ref {r['cand_scores'].tolist()}")
        assert not np.isnan(cs[s]).any(), (tag, s, cs[s])
        assert (cs[s][1:] <= cs[s][:-1]).all(), (tag, s, "scores increase", cs[s])
        assert np.array_equal(ct[s], r["cand_tokens"]) and np.array_equal(cb[s], r["cand_beams"]), \
            (tag, s, "tokens", ct[s], r["cand_tokens"], "beams", cb[s], r["cand_beams"], cs[s], r["cand_scores"])
        inf = r["cand_scores"] == -np.inf
        assert (cs[s][inf] == -np.inf).all() and np.isfinite(cs[s][~inf]).all(), (tag, s, cs[s], r["cand_scores"])
        if (~inf).any():
            err = np.abs(cs[s][~inf].astype(np.float64) - r["cand_scores"][~inf])
            bound = r["bound"][r["order"][:K]][~inf]
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (tag, s, "score error over the bound", err, bound)
    return worst


def _group(kw):
    return (kw["special"] or kw["place"]) + ("" if kw["vocab"] < 50000 else "-50265")


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("pid,kw", PARAMS, ids=[p for p, _ in PARAMS])
def test_candidates_against_the_reference(ctx, pid, kw, f16):
    case = R.make_case(f16, **kw)
    tag = f"{'f16' if f16 else 'f32'}/{pid}"
    ratio = _check_lists(tag, R.reference(case), *_candidates(ctx, case))
    print(f"{tag}: max err / bound {ratio:.3f}")
    key = f"{'f16' if f16 else 'f32'}/candidates/{_group(kw)}"
    _report(key, max(ratio, ERRORS.get(key, 0.0)), ERRORS, "beam_errors.json")


# ------------------------------------------------------------------------------------------------------------------ the search
def _search(ctx, p, f16=False, logits=None, lists=None, extra=0):
    """one mhip_beam_search_host call -> the trace as a dict of arrays, per-step ones cut to the steps that ran"""
    from marie_icr_amd._lib import BeamTrace, check

    bsz, beam, ML = p["bsz"], p["beam"], p["max_len"]
    S, M, K2 = ML + 1, bsz * beam, 2 * beam
    shapes = {"cand_scores": ((S, bsz, K2), np.float32), "cand_tokens": ((S, bsz, K2), np.int32), "cand_beams": ((S, bsz, K2), np.int32),
              "parent": ((S, M), np.int32), "last_tok": ((S, M), np.int32), "cum": ((S, M), np.float32), "ignore": ((S, M), np.uint8),
              "finished": ((S, bsz), np.uint8), "fin_count": ((S, bsz), np.int32), "tokens": ((S, M, ML + 2), np.int32),
              "anc": ((S, M, ML + 2), np.int32), "remaining": ((S,), np.int32), "fin_tokens": ((bsz, beam, ML + 1), np.int32),
              "fin_len": ((M,), np.int32), "fin_score": ((M,), np.float32), "out_tokens": ((bsz, ML + 1), np.int32),
              "out_len": ((bsz,), np.int32), "out_score": ((bsz,), np.float32)}
    tr = {k: np.zeros(sh, dt) for k, (sh, dt) in shapes.items()}
    bt = BeamTrace(**{k: tr[k].ctypes.data for k in shapes}, steps=-1)
    if logits is not None:
        logits = np.ascontiguousarray(logits)
        assert logits.shape == (S, M, p["ld"]) and logits.dtype == (np.float16 if f16 else np.float32)
        args = (vp(logits), NULL, NULL, NULL)
    else:
        ls = [np.ascontiguousarray(a, dt) for a, dt in zip(lists, (np.float32, np.int32, np.int32))]
        assert all(a.shape == (S, bsz, K2) for a in ls)
        args = (NULL, vp(ls[0]), vp(ls[1]), vp(ls[2]))
    rc, launches = _launches(ctx, lambda: ctx.lib.mhip_beam_search_host(
        ctx.h, int(f16), *args, ML, p["min_len"], p["pad"], p["eos"], p["vocab"], p["ld"], beam, bsz, extra, C.byref(bt)))
    check(ctx.h, rc, "mhip_beam_search_host")
    n = bt.steps
    assert 1 <= n <= S
    # init + per step (ancestry from step 1) + candidates (logits mode) + select + best
    assert launches == 1 + n * (2 if logits is not None else 1) + (n - 1) + 1, (launches, n)
    for k in R.PER_STEP:
        assert not tr[k][n:].any(), f"{k}: rows of steps that did not run were written"
        tr[k] = tr[k][:n]
    tr["steps"] = n
    return tr


def _assert_same_search(tag, dev, ref, beam):
    a, b = R.compared(dev, beam), R.compared(ref, beam)
    for k in R.differing(a, b):
        if a[k].shape != b[k].shape:
            pytest.fail(f"{tag}: {k}: device {a[k].shape}, reference {b[k].shape}")
        where = np.argwhere(a[k] != b[k])[0].tolist()
        pytest.fail(f"{tag}: {k} differs first at {where} (step first for per-step arrays): device {a[k][tuple(where)]}, "
                    f"reference {b[k][tuple(where)]}; {len(np.argwhere(a[k] != b[k]))} cells differ")


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("beam,bsz", R.SEARCH_SHAPES, ids=[f"beam{b}-bsz{n}" for b, n in R.SEARCH_SHAPES])
def test_search_on_scripted_logits(ctx, beam, bsz, f16):
    p, L, done_at = R.make_search(beam, bsz, f16)
    tag = f"{'f16' if f16 else 'f32'}/search-beam{beam}-bsz{bsz}"
    ML = p["max_len"]
    dev = _search(ctx, p, f16, logits=L)
    assert dev["steps"] == ML + 1
    # every step's lists, against the reference on the cum the device itself held
    worst, step_bound = 0.0, np.zeros((dev["steps"], bsz))
    for t in range(dev["steps"]):
        live = [s for s in range(bsz) if t == 0 or not dev["finished"][t - 1, s]]
        cum = np.zeros(bsz * beam, np.float32) if t == 0 else np.nan_to_num(dev["cum"][t - 1], nan=0.0, posinf=0.0, neginf=0.0)
        ref = R.candidates(L[t], cum, t, ML, p["min_len"], p["pad"], p["eos"], p["vocab"], beam, bsz)
        worst = max(worst, _check_lists(f"{tag} step {t}", ref, dev["cand_scores"][t], dev["cand_tokens"][t], dev["cand_beams"][t], live))
        for s in live:
            step_bound[t, s] = ref[s]["bound"][ref[s]["order"][:2 * beam]].max()
    _report(f"{'f16' if f16 else 'f32'}/search/beam{beam}-bsz{bsz}", worst, ERRORS, "beam_errors.json")
    # select, ancestry and best, fed the device's own lists
    forced = R.search(p, lists=(dev["cand_scores"], dev["cand_tokens"], dev["cand_beams"]), steps=dev["steps"])
    _assert_same_search(tag, dev, forced, beam)
    # the free-running fp64 search: same hypotheses; a score of length n carries at most the bounds of its n steps
    free = R.search(p, logits=L, dtype=np.float64)
    assert free["steps"] == dev["steps"]
    assert np.array_equal(dev["out_tokens"], free["out_tokens"]) and np.array_equal(dev["out_len"], free["out_len"])
    assert np.array_equal(dev["finished"], free["finished"]) and np.array_equal(dev["fin_count"], free["fin_count"])
    for s in range(bsz):
        n = int(dev["out_len"][s])
        assert n == min(done_at[s], ML) + 1 if R.crop_kind(s, bsz) != "one_per_step" else n >= 2
        bound = step_bound[:n, s].sum() / n + R.U32 * abs(free["out_score"][s])      # + the rounding of the division
        assert abs(float(dev["out_score"][s]) - free["out_score"][s]) <= bound, (tag, s, dev["out_score"][s], free["out_score"][s], bound)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_steps_enqueued_past_the_end_change_nothing(ctx, f16):
    """trocr_decode reads the counter two steps late and so enqueues one step past the end; here a batch that ends at step 3 of 6
    runs two, steps 4 and 5, on NaN logits"""
    beam, bsz = 3, 5
    p, L, done_at = R.make_search(beam, bsz, f16, late=False)
    assert done_at.max() == 3 and np.isnan(L[4:]).all()
    dev = _search(ctx, p, f16, logits=L, extra=0)
    more = _search(ctx, p, f16, logits=L, extra=2)
    assert dev["steps"] == 4 and more["steps"] == 6
    assert (more["remaining"][3:] == 0).all() and (more["finished"][3:] == 1).all()
    assert (more["parent"][3:] == np.arange(bsz * beam)).all() and (more["last_tok"][3:] == p["eos"]).all()
    assert np.array_equal(more["fin_count"][3:], np.repeat(dev["fin_count"][3:4], 3, axis=0))
    cut = dict(more, steps=4, **{k: more[k][:4] for k in R.PER_STEP})
    _assert_same_search("extra steps", cut, dev, beam)
    for k in ("fin_tokens", "fin_len", "fin_score", "out_tokens", "out_len", "out_score"):
        assert dev[k].tobytes() == more[k].tobytes(), k
    forced = R.search(p, lists=(more["cand_scores"], more["cand_tokens"], more["cand_beams"]), steps=6)
    _assert_same_search("extra steps, all six", more, forced, beam)


@pytest.mark.parametrize("name", sorted(R.list_cases()))
def test_search_on_hand_written_lists(ctx, name):
    p, lists = R.list_cases()[name]
    dev = _search(ctx, p, lists=lists)
    for k, a in zip(("cand_scores", "cand_tokens", "cand_beams"), lists):
        assert dev[k].tobytes() == np.ascontiguousarray(a[:dev["steps"]]).tobytes(), k
    _assert_same_search(name, dev, R.search(p, lists=lists), p["beam"])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_what_the_entries_cannot_run_is_refused(ctx):
    from marie_icr_amd._lib import BeamTrace, MarieHipError, check

    base = dict(step=1, max_len=6, min_len=1, pad=1, eos=2, vocab=24, ld=24, beam=3, bsz=2)
    L = np.zeros((6 * 4, 64), np.float32)
    cum = np.zeros(6 * 4, np.float32)
    outs = [np.full(64, 7, dt) for dt in (np.float32, np.int32, np.int32)]
    lists = [np.zeros((7, 2, 8), dt) for dt in (np.float32, np.int32, np.int32)]
    big = [np.zeros(7 * 8 * 64, np.int32) for _ in range(18)]
    bad = (("beam 0", dict(beam=0)), ("beam 5", dict(beam=5)), ("vocab < 2 * beam", dict(vocab=5, ld=8)),
           ("pitch no multiple of 8", dict(ld=28)), ("pitch below the vocabulary rounded up", dict(vocab=25, ld=24)),
           ("min_len > max_len", dict(min_len=7)), ("bsz 0", dict(bsz=0)))

    def cand(kw, ptrs=None):
        a = ptrs or (vp(L), vp(cum), vp(outs[0]), vp(outs[1]), vp(outs[2]))
        return ctx.lib.mhip_beam_candidates_host(ctx.h, 0, a[0], a[1], kw["step"], kw["max_len"], kw["min_len"], kw["pad"], kw["eos"],
                                                 kw["vocab"], kw["ld"], kw["beam"], kw["bsz"], a[2], a[3], a[4])

    def srch(kw, logits=True, trace=None, null_member=None, extra=0):
        bt = BeamTrace(**{n: (0 if n == null_member else big[i].ctypes.data) for i, (n, _) in enumerate(BeamTrace._fields_[:18])}, steps=-7)
        a = (vp(L), NULL, NULL, NULL) if logits else (NULL, vp(lists[0]), vp(lists[1]), vp(lists[2]))
        if logits is None:
            a = (NULL, vp(lists[0]), NULL, vp(lists[2]))
        rc = ctx.lib.mhip_beam_search_host(ctx.h, 0, *a, kw["max_len"], kw["min_len"], kw["pad"], kw["eos"], kw["vocab"], kw["ld"],
                                           kw["beam"], kw["bsz"], extra, NULL if trace is NULL else C.byref(bt))
        assert bt.steps == -7
        return rc

    calls = [(f"candidates: {what}", lambda kw=kw: cand(dict(base, **kw))) for what, kw in bad]
    calls += [(f"search: {what}", lambda kw=kw: srch(dict(base, **kw))) for what, kw in bad]
    calls += [(f"search, lists: {what}", lambda kw=kw: srch(dict(base, **kw), logits=False)) for what, kw in bad]
    full = (vp(L), vp(cum), vp(outs[0]), vp(outs[1]), vp(outs[2]))
    calls += [(f"candidates: null pointer {i}", lambda i=i: cand(base, tuple(NULL if j == i else full[j] for j in range(5)))) for i in range(5)]
    calls += [("candidates: step -1", lambda: cand(dict(base, step=-1))),
              ("search: no trace", lambda: srch(base, trace=NULL)), ("search: a null list", lambda: srch(base, logits=None)),
              ("search: a null member", lambda: srch(base, null_member="anc")), ("search: 3 extra steps", lambda: srch(base, extra=3))]
    lists[2][3, 1, 2] = 3         # a candidate naming beam 3 of 3
    calls += [("search, lists: a beam out of range", lambda: srch(base, logits=False))]
    for what, call in calls:
        with pytest.raises(MarieHipError):
            check(ctx.h, call(), what)
            pytest.fail(f"accepted: {what}")
    assert all((o == 7).all() for o in outs), "a refused call wrote output"
    assert not any(b.any() for b in big), "a refused search wrote output"
    lists[2][3, 1, 2] = 0
    assert cand(base) == 0 and not (outs[1][:12] == 7).any()          # and the same arguments, valid, run
