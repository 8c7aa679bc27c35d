"""Kernel-level parity of the flash attention kernels (csrc/attn_flash.hip: attn_flash_f16_kernel<>, <BiasArgs> and
attn_simple_f32_kernel<>, <BiasArgs>), one launch through mhip_attention_host with the whole descriptor in the test's hands,
against fp64 softmax attention of the exact operands the device received (oracle/attn_flash_ref.py, where both bounds are derived
from u16 = 2^-11, u32 = 2^-24 and magnitudes of the reference — nothing is fitted to the kernel):

    f16    |d| <= ((u16 + ln2 ds + 2^-21) B + 2^-25 V1) / (1 - rel) + (n_keys + ntiles + 4) u32 (A + |ref|) + u16 |ref| + 2^-25
    fp32   |d| <= (ln2 ds32 + 2^-21) B / (1 - rel) + (3 ntiles + 12) u32 (A + |ref|) + u32 |ref|
    and the mean forms (sqrt(K) for every accumulation length K, root-sum-square P roundings), as mean(err) <= mean(bound)

Cases (tests/test_oracle_attn_flash.py asserts the coverage, and that each named kernel bug moves the reference by >= 10 bounds):
n_keys 1, 8, 63, 64, 65, 128, 129, 193, 577 and n_queries 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257 in the fused (q | k rows) and
the split layout, heads 1 / 2 / 12 / 16, 1 .. 3 images, pitches ceil8(n) and ceil8(n) + 8, npad_q 264 over 100 queries, block counts 1, 3,
7, 8, 9, 15, 17, 25; nine softmax trajectories on a two-image, two-head, five-tile shape; the biased form at n 65 / 197 / 264 with a
different mask per image, dp / dx 7 / 9 and 511 / 1000, a wholly masked first or middle tile, masked keys under a rescale.  Padding
rows hold heavy finite values, the output buffer is pre-filled with the byte 0xff (NaN).

Isolation, bit for bit in both precisions: an image alone, a head alone, fused against split, heavy against zero padding and
slack, a query against the rescales of its wave's neighbours.

Measured on MI355X, worst error / bound over the 65 cases (per element; mean form):
    f16   plain 0.914; 0.355     biased 0.921; 0.275     (the CPU emulation of the f16 kernel's arithmetic: 0.921 at most)
    fp32  plain 0.124; 0.082     biased 0.096; 0.059
No kernel defect was found; 144 tests, 6.0 s for the file."""
import functools

import numpy as np
import pytest

from oracle import attn_flash_ref as R

pytestmark = pytest.mark.gpu

PARAMS = dict(R.all_params() + R.isolation_params())
PRECS = ("f16", "f32")


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _case(pid):
    case = R.build((pid, PARAMS[pid]))
    ref = R.reference(case)
    return case, {"f16": ref, "f32": dict(ref, hard=ref["hard32"], mean=ref["mean32"])}


def _prec(name):
    from marie_icr_amd._lib import PREC_F16, PREC_F32

    return PREC_F16 if name == "f16" else PREC_F32


def _launch(ctx, case, prec, **over):
    """one mhip_attention_host call under the launch profile -> the device's whole output in its element type"""
    from marie_icr_amd.layoutlmv3 import attention_host

    a = dict(case, **over)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        try:
            out = attention_host(ctx, _prec(prec), a["layout"], a["images"], a["heads"], a["n_queries"], a["n_keys"], a["npad_q"],
                                 a["npad_k"], a["q"], a["k"], a["vt"], a["bias"])
        finally:
            prof = ctx.profile_read()
            _launch.launches = {k: prof[k]["launches"] for k in ("attn_flash", "attn_bias")}
    finally:
        ctx.profile_enable(False)
    assert _launch.launches == ({"attn_flash": 1, "attn_bias": 0} if a["bias"] is None else {"attn_flash": 0, "attn_bias": 1})
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _untouched(a):
    return bool((_bits(a) == (0xffff if a.dtype == np.float16 else 0xffffffff)).all())


def _check_writes(case, prec, out):
    """the guard rows and the rows no block / no query covers keep the pre-fill, bit for bit"""
    images, nq, npq = case["images"], case["n_queries"], case["npad_q"]
    assert out.shape == (images * npq + R.SLACK, case["heads"] * 64)
    assert _untouched(out[images * npq:]), "a write behind the last image"
    first_free = min(npq, R.nqb(nq) * R.QB) if prec == "f16" else nq          # the fp32 kernel writes its queries only
    rows = out[:images * npq].reshape(images, npq, -1)
    assert _untouched(rows[:, first_free:]), "a write to rows beyond the launched query blocks"


def _judge(case, ref, out, what):
    got = R.judged_rows(case, out).astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: unwritten or non-finite elements in rows < n_queries"
    err = np.abs(got - ref["ref"])
    r = (float((err / ref["hard"]).max()), float(err.mean() / ref["mean"].mean()))
    print(f"{what}: max err / bound {r[0]:.3f}, mean err / mean bound {r[1]:.3f}")
    return r


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pid", [p for p, _ in R.all_params()])
def test_kernel_against_fp64_of_its_own_operands(ctx, pid, prec):
    case, refs = _case(pid)
    out = _launch(ctx, case, prec)
    _check_writes(case, prec, out)
    hard, mean = _judge(case, refs[prec], out, f"{pid} {prec}")
    assert hard <= 1.0, (pid, prec, hard)
    assert mean <= 1.0, (pid, prec, mean)


@pytest.mark.parametrize("prec", PRECS)
def test_a_shift_of_all_scores_changes_nothing(ctx, prec):
    """+200 / -200 / +0 log2 units on every score through one q . k component: the same outputs within the two bounds"""
    ids = {kw["variant"]: p for p, kw in R.variant_params()}
    outs, hard = {}, {}
    for v in ("shift_zero", "shift_plus", "shift_minus"):
        case, refs = _case(ids[v])
        outs[v] = R.judged_rows(case, _launch(ctx, case, prec)).astype(np.float64)
        hard[v] = refs[prec]["hard"]
    for v in ("shift_plus", "shift_minus"):
        d = np.abs(outs[v] - outs["shift_zero"])
        assert (d <= hard[v] + hard["shift_zero"]).all(), (v, float((d / (hard[v] + hard["shift_zero"])).max()))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pid", [p for p, _ in R.isolation_params()])
def test_an_image_a_head_and_a_layout_depend_on_nothing_but_their_own_operands(ctx, pid, prec):
    case, _ = _case(pid)
    images, heads, nq, npq = case["images"], case["heads"], case["n_queries"], case["npad_q"]
    base = _launch(ctx, case, prec)
    assert _same(base, _launch(ctx, case, prec)), "the same call twice differs"
    jb = R.judged_rows(case, base)
    for i in range(images):                      # each image alone: behind it lies the slack, not the next image
        alone = _launch(ctx, R.take_image(case, i), prec)
        assert _same(alone[:nq], jb[i]), f"image {i} alone differs from its rows of the batched call"
    for h in range(heads):
        one = R.take_head(case, h)
        alone = R.judged_rows(one, _launch(ctx, one, prec))
        assert _same(alone, np.ascontiguousarray(jb[..., h * 64:(h + 1) * 64])), f"head {h} alone differs from its columns"
    if case["npad_q"] == case["npad_k"]:
        other = R.SPLIT if case["layout"] == R.FUSED else R.FUSED
        assert _same(R.judged_rows(case, _launch(ctx, case, prec, layout=other)), jb), "fused and split layouts differ"
    zero = R.zero_padding(case)
    assert not np.array_equal(zero["q"], case["q"]) and not np.array_equal(zero["k"], case["k"]) and not np.array_equal(zero["vt"], case["vt"])
    assert _same(R.judged_rows(case, _launch(ctx, zero, prec)), jb), "a judged element depends on padding rows or slack"


@pytest.mark.parametrize("prec", PRECS)
def test_a_query_does_not_depend_on_the_rescales_of_its_wave(ctx, prec):
    """split_wave: the odd queries of every wave move their reference in tile 2; the even queries' results are bit for bit
    those of the call in which nobody moves"""
    pid = [p for p, kw in R.variant_params() if kw["variant"] == "split_wave"][0]
    case, _ = _case(pid)
    flat = R.make_case(**dict(PARAMS[pid], rise=False))
    nq = case["n_queries"]
    assert np.array_equal(flat["q"][0:nq:2], case["q"][0:nq:2]) and not np.array_equal(flat["q"][1:nq:2], case["q"][1:nq:2])
    a = R.judged_rows(case, _launch(ctx, case, prec))
    b = R.judged_rows(flat, _launch(ctx, flat, prec))
    assert _same(np.ascontiguousarray(a[:, 0::2]), np.ascontiguousarray(b[:, 0::2])), "an even query changed with its neighbours' rescale"
    assert not _same(np.ascontiguousarray(a[:, 1::2]), np.ascontiguousarray(b[:, 1::2]))


def _zeros(images, heads, npq, npk, biased):
    D = max(heads, 0) * 64
    rq, rk = max(images * npq, 0) + R.SLACK, max(images * npk, 0) + R.SLACK
    bias = None
    if biased:
        bias = dict(qcode=np.zeros((rq, 3), np.int32), kcode=np.concatenate([np.zeros((rk, 3), np.int32), np.ones((rk, 1), np.int32)], 1),
                    w1=np.zeros((heads, R.BINS_1D), np.float32), wx=np.zeros((heads, R.BINS_2D), np.float32),
                    wy=np.zeros((heads, R.BINS_2D), np.float32), max_1d=R.MAX_1D, max_2d=R.MAX_2D, dp=4, dx=4)
    return dict(q=np.zeros((rq, D), np.float32), k=np.zeros((rk, D), np.float32), vt=np.zeros(D * (rk - R.SLACK) + R.SLACK, np.float32), bias=bias)


@pytest.mark.parametrize("prec", PRECS)
def test_what_the_kernels_cannot_run_is_refused_without_a_launch(ctx, prec):
    from marie_icr_amd._lib import MarieHipError

    ok = dict(layout=R.SPLIT, images=2, heads=2, n_queries=10, n_keys=20, npad_q=16, npad_k=24)
    for biased in (False, True):
        _launch(ctx, dict(ok, **_zeros(2, 2, 16, 24, biased)), prec)                     # the base itself is accepted
        bad = [("npad_k % 8", dict(ok, npad_k=28)), ("n_queries > npad_q", dict(ok, n_queries=17)), ("n_keys > npad_k", dict(ok, n_keys=25)),
               ("no image", dict(ok, images=0)), ("no head", dict(ok, heads=0)), ("no key", dict(ok, n_keys=0)),
               ("no query", dict(ok, n_queries=0)), ("fused with two pitches", dict(ok, layout=R.FUSED))]
        for what, kw in bad + ([("dp 1024", "dp"), ("dx 1024", "dx")] if biased else []):
            if isinstance(kw, str):
                ops = _zeros(2, 2, 16, 24, True)
                ops["bias"][kw] = 1024
                kw = ok
            else:
                ops = _zeros(kw["images"], kw["heads"], kw["npad_q"], kw["npad_k"], biased)
            with pytest.raises(MarieHipError, match=r"\(-22\)"):
                _launch(ctx, dict(kw, **ops), prec)
                pytest.fail(f"accepted: {what}")
            assert _launch.launches == {"attn_flash": 0, "attn_bias": 0}, (what, _launch.launches)
