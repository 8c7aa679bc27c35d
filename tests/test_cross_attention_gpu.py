"""Kernel-level parity of the decoder's encoder-attention with absorbed projections (csrc/cross_attn.hip: absorb_q_kernel,
cross_attn_kernel<ED, W>, absorb_v_kernel), each kernel alone through mhip_cross_attention_stages_host, against fp64 of the exact
operands that kernel received (oracle/cross_attention_ref.py, where every bound is derived from u16 = 2^-11, u32 = 2^-24 and
magnitudes of the reference — nothing is fitted to the kernel):

    absorb_q    against W_kt^T q in fp64                       |d| <= u16 |ref| + 2^-25 + (64 + 4) u32 (|q| |W_kt|)
    cross_attn  against softmax2(qt_dev . E) E in fp64         |d| <= rel A + 2^-25 sum |E| / L + u16 |ref| + 2^-25
    absorb_v    against W_v ct_dev + b_v in fp64               |d| <= u16 |ref| + 2^-25 + (ED + 4) u32 (|ct| |W_v|^T + |b_v|)
    end to end  against fairseq's MultiheadAttention in fp64   the three bounds propagated (loose: the one overall check)
    and the mean forms (sqrt(K) for K), as mean(err) <= mean(bound)

Cases (tests/test_oracle_cross_attention.py asserts the coverage on the CPU): all 16 instantiations ED {256, 512, 768, 1024} x
beam {1, 2, 3, 4}, each against n_keys 1, 31, 32, 33, 32 DEPTH, 32 DEPTH + 1, 32 (DEPTH + 1) + 1 and 577 (fewer tiles than the ring
is deep, exactly as many, one and two feeding tiles, the product's 19); heads 1 / 4 / 12 / 16, 1 .. 3 crops and crop pitches npad /
npad + 8 rotated through them; per ED one call of 17 crops x beam 4 (68 rows: a full and a partial 64-row block of the absorb
kernels) and seven softmax trajectories (a late dominant key, tile maxima rising by 7, the maximum in tile 0, identical keys, all
scores shifted by +-200).  The caller's padding rows hold 1.5 x the crop's heaviest key, the scratch is pre-filled with NaN.  The
CPU test proves that dropping the first / last / 31st / 32nd key, admitting key n_keys, swapping two heads, reading beam 0's
queries or crop 0's tokens everywhere, or losing a rescale moves the reference by >= 10 bounds.

Isolation, bit for bit, on three shapes per ED: a crop run alone, finite 6e4 in everything the kernel reads masked (padding rows,
the next crop's first rows), another beam's queries changed, the same call twice.

Measured on MI355X, worst error / bound over the 152 cases (per element; mean form), per ED 256 / 512 / 768 / 1024:
    absorb_q    0.975 / 0.976 / 0.979 / 0.978;  0.49 / 0.48 / 0.48 / 0.48    (the maxima sit where the f16 store is the whole bound)
    cross_attn  0.465 / 0.273 / 0.196 / 0.137;  0.20 / 0.19 / 0.33 / 0.23    (the CPU emulation of its arithmetic: 0.47 at most)
    absorb_v    0.887 / 0.817 / 0.639 / 0.572;  0.37 / 0.38 / 0.36 / 0.34
    end to end  0.029 / 0.014 / 0.009 / 0.005;  0.023 / 0.025 / 0.026 / 0.026
No kernel defect was found; 169 tests, 17 s for the file.

The ratios are written to cross_attention_errors.json beside the other parity reports (test_fullsize_gpu._report)."""
import ctypes as C

import numpy as np
import pytest

from oracle import cross_attention_ref as R
from test_fullsize_gpu import _report

pytestmark = pytest.mark.gpu

ERRORS = {}
PARAMS = dict(R.all_params() + R.isolation_params())


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _call(ctx, q, E, wk, wv, bv, crops, beam, heads, n_tok, kv_rows, ed, out=None):
    """one mhip_cross_attention_stages_host call under the launch profile -> (qt, ct [M][16][ed], out [M][D], launches by kernel)"""
    from marie_icr_amd._lib import check

    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                      # noqa: E731
    arrs = [np.ascontiguousarray(a, np.float32) for a in (q, E, wk, wv, bv)]
    M = max(1, crops * beam)
    qt = np.zeros((M, 16, max(ed, 1)), np.float32)
    ct = np.zeros_like(qt)
    out = np.zeros((M, max(heads, 1) * 64), np.float32) if out is None else out
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        rc = ctx.lib.mhip_cross_attention_stages_host(ctx.h, *(vp(a) for a in arrs), crops, beam, heads, n_tok, kv_rows, ed, vp(qt),
                                                      vp(ct), vp(out))
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    launches = {k: prof[k]["launches"] for k in ("cross_attn", "dec_ops")}
    _call.launches = launches              # also for the caller of a refused call
    check(ctx.h, rc, "mhip_cross_attention_stages_host")
    return qt, ct, out, launches


def _run(ctx, case, q=None, E=None, crops=None):
    q = case["q"] if q is None else q
    E = case["E"] if E is None else E
    crops = case["crops"] if crops is None else crops
    qt, ct, out, launches = _call(ctx, q, E, case["wk"], case["wv"], case["bv"], crops, case["beam"], case["heads"], case["n_keys"],
                                  case["kv_rows"], case["ed"])
    assert launches == {"cross_attn": 1, "dec_ops": 2}, launches
    return qt, ct, out


def _same(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def _judge(pid, stage, got, ref, hard, mean):
    err = np.abs(got.astype(np.float64) - ref)
    r = {"max_err_over_bound": float((err / hard).max()), "mean_err_over_mean_bound": float(err.mean() / mean.mean())}
    ERRORS.setdefault(pid, {})[stage] = r
    return r


@pytest.mark.parametrize("pid", [p for p, _ in R.all_params()])
def test_each_kernel_against_fp64_of_its_own_operands(ctx, pid):
    case = R.make_case(**PARAMS[pid])
    heads = case["heads"]
    qt, ct, out = _run(ctx, case)
    # what the kernels wrote: head slots >= heads still hold the pre-filled NaN, everything else is finite
    for name, tap in (("qt", qt), ("ct", ct)):
        assert np.isnan(tap[:, heads:]).all(), f"{name}: head slots >= heads were written"
        assert np.isfinite(tap[:, :heads]).all(), f"{name}: unwritten or non-finite elements"
    assert np.isfinite(out).all(), "unwritten or non-finite output elements"
    R.assert_trajectory(case, qt)
    st = R.stages(case, qt, ct)
    rs = [_judge(pid, "qt", qt[:, :heads], st["qt_ref"], st["qt_hard"], st["qt_mean"]),
          _judge(pid, "ct", ct[:, :heads], st["ct_ref"], st["ct_hard"], st["ct_mean"]),
          _judge(pid, "ao", out, st["ao_ref"], st["ao_hard"], st["ao_mean"]),
          _judge(pid, "e2e", out, st["e2e_ref"], st["e2e_hard"], st["e2e_mean"])]
    _report(pid, ERRORS[pid], ERRORS, "cross_attention_errors.json")
    print(pid, " ".join(f"{s} {r['max_err_over_bound']:.3f}/{r['mean_err_over_mean_bound']:.3f}" for s, r in zip(("qt", "ct", "ao", "e2e"), rs)))
    for stage, r in zip(("qt", "ct", "ao", "e2e"), rs):
        assert r["max_err_over_bound"] <= 1.0, (pid, stage, r)
        assert r["mean_err_over_mean_bound"] <= 1.0, (pid, stage, r)
    if case["variant"] == "identical":
        want = np.repeat(case["E"][:, 0], case["beam"], axis=0)[:, None, :]
        assert (np.abs(ct[:, :heads] - want) <= st["ct_hard"]).all(), "identical keys: the context is that key"


@pytest.mark.parametrize("ed", R.EDS)
def test_a_shift_of_all_scores_changes_nothing(ctx, ed):
    """+200 / -200 / +0 log2 units on every score through component ed - 1 of qt: the same contexts within the two bounds"""
    ids = {v: p for p, kw in R.variant_params() if kw["ed"] == ed for v in (kw["variant"],)}
    cases = {v: R.make_case(**PARAMS[ids[v]]) for v in ("shift_zero", "shift_plus", "shift_minus")}
    heads = cases["shift_zero"]["heads"]
    taps = {v: _run(ctx, c) for v, c in cases.items()}
    hard = {v: R.ct_stage(cases[v], taps[v][0])["hard"] for v in cases}
    for v in ("shift_plus", "shift_minus"):
        assert _same(taps[v][0][:, :heads, :-1], taps["shift_zero"][0][:, :heads, :-1])
        d = np.abs(taps[v][1][:, :heads].astype(np.float64) - taps["shift_zero"][1][:, :heads])
        assert (d <= hard[v] + hard["shift_zero"]).all(), (v, float((d / (hard[v] + hard["shift_zero"])).max()))


@pytest.mark.parametrize("pid", [p for p, _ in R.isolation_params()])
def test_a_crop_and_a_beam_depend_on_nothing_but_their_own_operands(ctx, pid):
    case = R.make_case(**PARAMS[pid])
    ed, beam, n, crops, kv = (case[k] for k in ("ed", "beam", "n_keys", "crops", "kv_rows"))
    base = _run(ctx, case)
    again = _run(ctx, case)
    for a, b, what in zip(base, again, ("qt", "ct", "out")):
        assert _same(a, b), f"the same call twice: {what} differs"
    rows = lambda t, c: t[c * beam:(c + 1) * beam]                                   # noqa: E731
    # each crop alone (the rows behind it are then the zero slack rows)
    for c in range(crops):
        alone = _run(ctx, case, q=rows(case["q"], c), E=case["E"][c:c + 1], crops=1)
        for a, b, what in zip(alone, base, ("qt", "ct", "out")):
            assert _same(a, rows(b, c)), f"crop {c} alone: {what} differs from its rows of the batched call"
    # everything the kernel reads masked behind crop c — its padding rows and the next crop's first rows, up to the end of the
    # tile after its last — replaced by finite values of magnitude 6e4 (finite: 0 x NaN would poison the second product)
    sign = np.where(np.arange(ed) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for c in range(crops):
        flat = case["E"].reshape(crops * kv, ed).copy()
        lo, hi = c * kv + n, min(crops * kv, c * kv + R.ntiles(n) * R.TK + R.TK)
        flat[lo:hi] = 6e4 * sign
        assert hi > lo or c == crops - 1
        got = _run(ctx, case, E=flat.reshape(crops, kv, ed))
        for a, b, what in zip(got, base, ("qt", "ct", "out")):
            assert _same(rows(a, c), rows(b, c)), f"crop {c}: {what} depends on rows behind its last key"
    # another beam's queries
    q2 = case["q"].reshape(crops, beam, -1).copy()
    q2[:, 1:] = R.f16(np.random.default_rng(7).normal(0, 0.5, q2[:, 1:].shape))
    got = _run(ctx, case, q=q2.reshape(case["q"].shape))
    for a, b, what in zip(got, base, ("qt", "ct", "out")):
        assert _same(a[0::beam], b[0::beam]), f"beam 0: {what} depends on another beam's queries"
        assert not _same(a[1::beam], b[1::beam])


def test_what_the_kernels_cannot_run_is_refused_without_a_launch(ctx):
    from marie_icr_amd._lib import MarieHipError

    ok = dict(crops=2, beam=3, heads=4, n_tok=33, kv_rows=40, ed=256)
    big = {k: np.zeros(s, np.float32) for k, s in (("q", (16, 17 * 64)), ("E", (2, 48, 1024)), ("wk", (17 * 64, 1024)), ("wv", (17 * 64, 1024)),
                                                   ("bv", (17 * 64,)))}
    _call(ctx, *big.values(), **ok)                                                 # the base itself is accepted
    for what, kw in (("enc_dim 384", dict(ok, ed=384)), ("beam 5", dict(ok, beam=5)), ("heads 17", dict(ok, heads=17)),
                     ("kv_rows < n_tok", dict(ok, kv_rows=32)), ("n_tok < 1", dict(ok, n_tok=0)), ("kv_rows % 8", dict(ok, kv_rows=44)),
                     ("crops < 1", dict(ok, crops=0))):
        out = np.full((16, 17 * 64), 7.0, np.float32)
        with pytest.raises(MarieHipError):
            _call(ctx, *big.values(), out=out, **kw)
            pytest.fail(f"accepted: {what}")
        assert _call.launches == {"cross_attn": 0, "dec_ops": 0}, (what, _call.launches)
        assert (out == 7.0).all(), f"{what}: a refused call wrote output"
