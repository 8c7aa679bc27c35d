"""Kernel-level parity of the decoder's decode attention (csrc/trocr_ops.hip, mhip_launch_decode_attention) through
mhip_decode_attention_host, against softmax attention in fp64 on the same rounded operands (oracle/decode_attention_ref.py).

The launcher picks one of three kernels by history length; the n_keys of the sweep straddle each hand-over:

    n_keys   1 .. 64      f16, heads % 8 == 0: decode_self_attn_f16_kernel (one key per lane: readlane(slot, s))
                          (also run with force_generic: the generic kernel over the same operands)
    n_keys   1 .. 256     decode_attn_kernel<T, 1, 256>: every fp32 step, f16 steps past 64 keys, heads 4 / 12
    n_keys 257 .. 640     decode_attn_kernel<T, 4, 640>: long histories, and the encoder-attention (nq > 1, 577 tokens)
    n_keys 641, nq 5      rejected (MarieHipError)

Self-attention operands come from a simulated beam search (ancestry tables through ancestry_kernel's recurrence), rows are
never a multiple of 4, the output is pre-filled with NaN, the encoder-attention's padding rows hold NaN.  The data is built so
that each row's softmax weight sits largely on one key — the last, the first, or one just past a 4-, 16-, 32- or 64-key
boundary — and tests/test_oracle_decode_attention.py proves on the CPU that dropping the first or last key, reading the ancestry
of step s +- 1, using row 0's ancestry for every row or swapping two heads moves the reference by >= 10 x the bars below.

Bars, relative to max(1, max |ref|): fp32 max |d| <= 2e-6; f16 max |d| <= 1e-3, mean |d| <= 1e-4 (the output is rounded to f16).
Measured on MI355X, worst case per path (max |d| / mean |d|, relative):

    f16  short-history kernel, 1 .. 64 keys          3.4e-4 / 4.5e-5     fp32  generic (1, 256), 1 .. 256 keys    5.0e-7 / 3.1e-8
    f16  generic forced, 1 .. 64 keys                3.4e-4 / 4.5e-5     fp32  generic (4, 640), 257 .. 640 keys  7.4e-7 / 3.0e-8
    f16  generic (1, 256), 1 .. 256 keys             4.1e-4 / 4.5e-5     fp32  encoder-attention, nq 1 / 3 / 4    7.8e-7 / 3.1e-8
    f16  generic (4, 640), 257 .. 640 keys           3.8e-4 / 3.6e-5
    f16  encoder-attention, nq 1 / 3 / 4             4.4e-4 / 4.0e-5

With MARIE_TEST_REPORT_DIR set, the measured errors are written to decode_attention_errors.json there."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import decode_attention_ref as R

pytestmark = pytest.mark.gpu

REPORT = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()
    d = os.environ.get("MARIE_TEST_REPORT_DIR")
    if d and os.path.isdir(d) and REPORT:
        with open(os.path.join(d, "decode_attention_errors.json"), "w") as f:
            json.dump(REPORT, f, indent=1, default=float)


def _run(ctx, case, f16, force_generic=False, rows=None):
    from marie_icr_amd._lib import PREC_F16, PREC_F32, check

    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)
    q = np.ascontiguousarray(case["q"], np.float32)
    k = np.ascontiguousarray(case["k"], np.float32)
    v = np.ascontiguousarray(case["v"], np.float32)
    anc = None if case["anc"] is None else np.ascontiguousarray(case["anc"], np.int32)
    rows = q.shape[0] if rows is None else rows
    out = np.empty((rows, case["heads"] * 64), np.float32)
    rc = ctx.lib.mhip_decode_attention_host(ctx.h, PREC_F16 if f16 else PREC_F32, case["heads"], case["n_keys"], case["nq"], rows,
                                            case["slots"], case["kv_rows"], vp(q), vp(k), vp(v), vp(anc),
                                            0 if anc is None else anc.shape[1], int(force_generic), vp(out))
    check(ctx.h, rc, "mhip_decode_attention_host")
    return out


def _compare(pid, out, ref, f16):
    assert np.isfinite(out).all(), f"{pid}: unwritten or non-finite output cells"
    d = np.abs(out.astype(np.float64) - ref)
    bmax, bmean = R.bars(f16, ref)
    REPORT[pid] = {"max": float(d.max()), "mean": float(d.mean()), "max_ref": float(np.abs(ref).max())}
    assert d.max() <= bmax, (pid, d.max(), bmax)
    assert d.mean() <= bmean, (pid, d.mean(), bmean)


@pytest.mark.parametrize("pid,kw", R.self_params(), ids=[p for p, _ in R.self_params()])
def test_self_attention_over_a_beam_history(ctx, pid, kw):
    case = R.self_case(**kw)
    ref = R.reference(case)
    fast = kw["f16"] and kw["n_keys"] <= R.DISPATCH[0] and kw["heads"] % 8 == 0
    _compare(pid + ("-fast" if fast else "-generic"), _run(ctx, case, kw["f16"]), ref, kw["f16"])
    if fast:
        _compare(pid + "-forced-generic", _run(ctx, case, kw["f16"], force_generic=True), ref, kw["f16"])


@pytest.mark.parametrize("pid,kw", R.cross_params(), ids=[p for p, _ in R.cross_params()])
def test_encoder_attention_over_projected_keys(ctx, pid, kw):
    """the fp32 / MARIE_HIP_NO_ABSORB form: nq queries per crop over the crop's first n_keys rows, NaN padding behind them"""
    case = R.cross_case(**kw)
    _compare(pid, _run(ctx, case, kw["f16"]), R.reference(case), kw["f16"])


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_what_the_kernels_cannot_run_is_rejected(ctx, f16):
    from marie_icr_amd._lib import MarieHipError

    too_long = R.self_case(seed=3, heads=8, n_keys=641, crops=1, beam=2, f16=f16)
    with pytest.raises(MarieHipError, match="n_keys 641"):
        _run(ctx, too_long, f16)
    enc = R.cross_case(seed=4, heads=8, n_keys=641, groups=2, nq=1, f16=f16)
    with pytest.raises(MarieHipError, match="n_keys 641"):
        _run(ctx, enc, f16)
    five = R.cross_case(seed=5, heads=8, n_keys=20, groups=2, nq=5, f16=f16)
    with pytest.raises(MarieHipError, match="nq 5"):
        _run(ctx, five, f16)
