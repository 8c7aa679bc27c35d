"""Kernel-level parity of the BiLSTM recurrence (csrc/lstm.hip: lstm_rec_resident_f16, lstm_rec_stream<float>, the packers
mhip_lstm_pack_whh / mhip_lstm_xproj_row) alone through mhip_lstm_rec_host, against a teacher-forced LSTM in fp64 on the same
rounded weights (oracle/lstm_ref.py): each step of the reference consumes the device's own h of the step before, so every step
is compared at rounding level and a wrong operand at any step — a stale buffer, the wrong row, a dropped k-step — shows at that
step at full size.

Every bar is the per-element bound oracle/lstm_ref.py derives from u16 = 2^-11, u32 = 2^-24 and the reference's magnitudes
(its docstring has the derivation); tests/test_oracle_lstm.py proves on the CPU that an emulation of the kernels' arithmetic
stays inside it and that six kernel bugs break it by 60 x to 10^7 x.  Per case, in both precisions and both directions:
    rows < B finite; the 16 guard rows behind them still hold the 0xff fill bit for bit; exactly one lstm_rec launch;
    |h_dev - h_ref| <= bound per element; mean error <= mean of the probabilistic bound (sqrt(256) for 256 + 1 in dpre).
The B = 33 case runs a second time with xproj rows 16 .. 32 replaced: rows 0 .. 15 must come out as the same bits.

The cases are oracle/lstm_ref.GPU_CASES: W_hh at the recognizers' scale (gain 1) and three times it, gate columns saturated at
+-40 in both signs, units whose |c| climbs to about T (62.7 at T = 63: exp2 overflows inside tanh(c)), an all-saturated case.

Measured on MI355X, max err / bound | mean err / mean bound:
    case                           f16                fp32
    B1-T1-gain1                 0.941 | 0.346      0.248 | 0.046
    B1-T1-gain3                 0.911 | 0.383      0.190 | 0.053
    B15-T2-gain1                0.951 | 0.359      0.256 | 0.042
    B15-T2-gain3                0.968 | 0.356      0.303 | 0.027
    B16-T3-gain1                0.965 | 0.357      0.320 | 0.038
    B16-T3-gain3                0.969 | 0.354      0.331 | 0.022
    B17-T24-gain1               0.974 | 0.350      0.322 | 0.029
    B17-T24-gain3               0.973 | 0.343      0.344 | 0.014
    B33-T63-gain1               0.963 | 0.349      0.329 | 0.028
    B33-T63-gain3               0.963 | 0.342      0.317 | 0.014
    B16-T63-gain3-saturated     0.374 | 0.329      0.153 | 0.053
The f16 maxima are the half-ulp rounding of h, which the bound meets; the device's figures equal the CPU emulation's to two digits.
With the f16 kernel's LDS-resident k-steps skipped for one u on a scratch build, every f16 case with T >= 2 but the saturated one
fails at 4.5e3 .. 1.3e4 x the bound; with both kernels streaming h out of buffer 0 whatever the parity, every case with T >= 2
fails at 5e4 x and more (the CPU test's zero_fragment and stale_h mutations predict 3e3 .. 1e5 x).

The ratios are written to lstm_errors.json beside the other parity reports (test_fullsize_gpu._report)."""
import ctypes as C

import numpy as np
import pytest

from oracle import lstm_ref as R
from test_fullsize_gpu import _report

pytestmark = pytest.mark.gpu

GUARD = 16                       # rows behind row B of the device's h buffer: one workgroup tile
ERRORS = {}
PARAMS = R.case_params()


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _run(ctx, whh, xproj, f16):
    """one mhip_lstm_rec_host call -> out [B + GUARD][T][512] fp32; asserts that exactly one lstm_rec kernel was launched"""
    from marie_icr_amd._lib import PREC_F16, PREC_F32, check

    B, T = xproj.shape[:2]
    whh = np.ascontiguousarray(whh, np.float32)
    xproj = np.ascontiguousarray(xproj, np.float32)
    assert whh.shape == (2, 4 * R.HID, R.HID) and xproj.shape == (B, T, 2, 4 * R.HID)
    out = np.zeros((B + GUARD, T, 2 * R.HID), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        rc = ctx.lib.mhip_lstm_rec_host(ctx.h, PREC_F16 if f16 else PREC_F32, B, T, vp(whh), vp(xproj), vp(out))
        check(ctx.h, rc, "mhip_lstm_rec_host")
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    assert prof["lstm_rec"]["launches"] == 1, prof["lstm_rec"]
    return out


def _fill(f16):
    """the 0xff fill as it comes back: f16 0xffff widens to the fp32 NaN 0xffffe000"""
    return np.uint32(0xFFFFE000 if f16 else 0xFFFFFFFF)


def _check(tag, out, whh, xproj, f16):
    B = xproj.shape[0]
    dev = out[:B]
    assert np.isfinite(dev).all(), f"{tag}: unwritten or non-finite cells in rows < B"
    assert (out[B:].view(np.uint32) == _fill(f16)).all(), f"{tag}: the guard rows behind row B were written"
    ref = R.reference_forced(R.rounded(whh, f16), xproj, dev, f16)
    err = np.abs(dev.astype(np.float64) - ref["h"])
    ratio = err / ref["bound"]
    r = {"max_err_over_bound": float(ratio.max()), "mean_err_over_mean_bound": float(err.mean() / ref["mean_bound"].mean()),
         "c_max": ref["c_max"]}
    _report(tag, r, ERRORS, "lstm_errors.json")
    print(f"{tag}: max err / bound {r['max_err_over_bound']:.3f}  mean err / mean bound {r['mean_err_over_mean_bound']:.3f}  "
          f"max |c| {ref['c_max']:.1f}")
    bad = np.argwhere(err > ref["bound"])
    assert bad.size == 0, (tag, "first element over the bound [b, t, dir * 256 + unit]", bad[0].tolist(), float(err[tuple(bad[0])]),
                           float(ref["bound"][tuple(bad[0])]), "elements over", len(bad), "worst ratio", r["max_err_over_bound"])
    assert err.mean() <= ref["mean_bound"].mean(), (tag, "mean error over the mean bound", r)
    return dev


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("pid,kw", PARAMS, ids=[p for p, _ in PARAMS])
def test_recurrence_against_the_forced_reference(ctx, pid, kw, f16):
    whh, xproj = R.make_case(**kw)
    tag = f"{'f16' if f16 else 'f32'}/{pid}"
    dev = _check(tag, _run(ctx, whh, xproj, f16), whh, xproj, f16)
    if kw["B"] == 33:
        # the recurrence is per batch row: other rows in the workgroups behind must not reach rows 0 .. 15
        other = R.replace_rows(xproj, 16)
        assert not np.array_equal(other[16:], xproj[16:]) and np.array_equal(other[:16], xproj[:16])
        again = _run(ctx, whh, other, f16)
        assert np.array_equal(again[:16].view(np.uint32), dev[:16].view(np.uint32)), f"{tag}: rows 0 .. 15 depend on rows 16 .. 32"
        assert not np.array_equal(again[16:33], dev[16:33])


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_what_the_entry_cannot_run_is_rejected(ctx, f16):
    from marie_icr_amd._lib import PREC_F16, PREC_F32, MarieHipError, check

    whh, xproj = R.make_case(1, 1, 1)
    out = np.zeros((1 + GUARD, 1, 2 * R.HID), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    prec = PREC_F16 if f16 else PREC_F32
    null = C.c_void_p(0)
    for what, args in (("B = 0", (prec, 0, 1, vp(whh), vp(xproj), vp(out))), ("T = 0", (prec, 1, 0, vp(whh), vp(xproj), vp(out))),
                       ("precision 7", (7, 1, 1, vp(whh), vp(xproj), vp(out))), ("no weights", (prec, 1, 1, null, vp(xproj), vp(out))),
                       ("no xproj", (prec, 1, 1, vp(whh), null, vp(out))), ("no out", (prec, 1, 1, vp(whh), vp(xproj), null))):
        with pytest.raises(MarieHipError):
            check(ctx.h, ctx.lib.mhip_lstm_rec_host(ctx.h, *args), "mhip_lstm_rec_host")
            pytest.fail(f"accepted: {what}")
    assert (out == 0).all(), "a refused call wrote output"
