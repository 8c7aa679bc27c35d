"""Kernel-level parity of the recognizer's non-GEMM kernels (csrc/icr_ops.hip), each alone through its stage entry
(mhip_*_host -> the launcher the ICR model calls) against the float64 statements of tests/icr_ops_ref.py.

Bars: the max-pool and the arg-max indices bitwise; fp32 mode max |kernel - fp64| <= 1e-3 on outputs the CPU test
asserts to be O(1); the same 1e-3 in the f16 mode, where the only f16 step of these kernels is the rounding of an output <= 2
(2^-11 * 2 = 4.9e-4) and the inputs are f16-representable; pmax to 1e-4 relative.  tests/test_icr_ops_ref_cpu.py shows without a
GPU that each mistake named there moves the reference by at least 50 bars on exactly these inputs.

First MI355X figures, max |kernel - fp64| over the cases of each kernel (bar 1e-3):
    kernel            fp32                 f16
    conv_gray_first   9.2e-08 .. 2.3e-07   2.9e-04 .. 4.9e-04
    avgpool_hw        0 .. 2.6e-08         2.1e-04 .. 2.4e-04
    tps_sample        7.2e-08 .. 3.4e-05   (fp32 only)
    attn_context      0 .. 5.4e-07         0 .. 4.9e-04
    attn_cell c, h    8.3e-08 .. 1.4e-07   h 2.4e-04 (c is fp32 in both modes)
    pmax (relative)   <= 1.5e-07           (fp32 only; bar 1e-4)

Every output comes back with STAGE_GUARD elements behind it, which must still hold the 0xff fill; the cells in front of them must
all have been written (the fill is NaN / -1)."""
import numpy as np
import pytest

import icr_ops_ref as R

pytestmark = pytest.mark.gpu
PRECS = ["f16", "f32"]


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def prec_of(name):
    from marie_icr_amd._lib import PREC_F16, PREC_F32

    return PREC_F16 if name == "f16" else PREC_F32


def split(out, shape, tag, widened_f16=False):
    """the output proper, after checking the guard behind it and that every cell in front was written"""
    from marie_icr_amd._lib import STAGE_GUARD

    n = int(np.prod(shape))
    assert out.size == n + STAGE_GUARD
    body, guard = out[:n].reshape(shape), out[n:]
    if out.dtype == np.float32:
        fill = np.uint32(0xFFFFE000 if widened_f16 else 0xFFFFFFFF)       # f16 0xffff widens to this fp32 NaN
        assert (guard.view(np.uint32) == fill).all(), f"{tag}: the guard behind the output was written"
    else:
        assert (guard == -1).all(), f"{tag}: the guard behind the output was written"
    return body


def close(tag, dev, ref, bar=R.BAR):
    assert np.isfinite(dev).all(), f"{tag}: unwritten or non-finite cells"
    err = float(np.abs(dev.astype(np.float64) - ref).max())
    print(f"{tag}: largest |ref| {np.abs(ref).max():.3f}  max err {err:.2e}  bar {bar:.1e}")
    assert np.abs(ref).max() <= 2.0
    assert err <= bar, (tag, err, bar)


def refused(fn, *args):
    from marie_icr_amd._lib import MarieHipError

    with pytest.raises(MarieHipError):
        fn(*args)


# ---------------------------------------------------------------------------------------------------------- conv_gray_first
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cid,kw", R.GRAY_CASES, ids=[c for c, _ in R.GRAY_CASES])
def test_conv_gray_first(ctx, cid, kw, prec):
    from marie_icr_amd.icr import conv_gray_first

    c = R.gray_case(**kw)
    ref = R.conv_gray_first(c["img"], c["w"], c["scale"], c["bias"])
    out = conv_gray_first(ctx, prec_of(prec), c["img"], c["w"], c["scale"], c["bias"])
    dev = split(out, ref.shape, cid, prec == "f16")
    close(f"conv_gray_first {prec} {cid}", dev, ref)
    assert (dev[..., kw["C"]:] == 0).all(), "channels >= C must be exactly zero"


def test_conv_gray_first_refuses(ctx):
    from marie_icr_amd.icr import conv_gray_first

    refused(conv_gray_first, ctx, prec_of("f32"), np.zeros((1, 3, 5), np.uint8), np.zeros((9, 65)), np.ones(65), np.zeros(65))


# ---------------------------------------------------------------------------------------------------------- pools
S21 = [(cid, shape, neg, p) for cid, shape, neg, precs in R.S21_CASES for p in precs]


@pytest.mark.parametrize("cid,shape,neg,prec", S21, ids=[f"{c[0]}-{c[3]}" for c in S21])
def test_maxpool_s21_p01(ctx, cid, shape, neg, prec):
    from marie_icr_amd.icr import maxpool_s21_p01

    x = R.pool_input(61, shape, neg)
    ref = R.maxpool_s21_p01(x).astype(np.float32)
    dev = split(maxpool_s21_p01(ctx, prec_of(prec), x), ref.shape, cid, prec == "f16")
    diff = int((dev.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"maxpool_s21_p01 {prec} {cid}: {diff} of {ref.size} outputs differ")
    assert diff == 0


@pytest.mark.parametrize("prec", PRECS)
def test_maxpool_s21_p01_refuses(ctx, prec):
    from marie_icr_amd.icr import maxpool_s21_p01

    refused(maxpool_s21_p01, ctx, prec_of(prec), np.zeros((1, 1, 4, 8), np.float32))       # H = 1: no output row
    refused(maxpool_s21_p01, ctx, prec_of(prec), np.zeros((1, 4, 4, 6), np.float32))       # C = 6: no whole vector


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", R.AVG_SHAPES, ids=str)
def test_avgpool_hw(ctx, shape, prec):
    from marie_icr_amd.icr import avgpool_hw

    x = R.avg_input(71, shape)
    ref = R.avgpool_hw(x)
    close(f"avgpool_hw {prec} {shape}", split(avgpool_hw(ctx, prec_of(prec), x), ref.shape, str(shape), prec == "f16"), ref)


# ---------------------------------------------------------------------------------------------------------- TPS
@pytest.mark.parametrize("cid,kw", R.TPS_CASES, ids=[c for c, _ in R.TPS_CASES])
def test_tps_sample(ctx, cid, kw):
    from marie_icr_amd.icr import tps_sample

    c = R.tps_case(**kw)
    args = (c["crops"], c["c_prime"], c["inv_delta_c"], c["p_hat"])
    ref = R.tps_sample(*args)
    dev = split(tps_sample(ctx, *args), ref.shape, cid)
    close(f"tps_sample {cid}", dev, ref)
    if kw["kind"] == "identity":
        # the identity fiducials: the crop as grid_sample reads pixel centres with align_corners=True, in closed form
        close(f"tps_sample {cid} vs the closed form", dev, R.tps_identity_expected(c["crops"]))


def test_tps_sample_refuses(ctx):
    from marie_icr_amd.icr import tps_sample

    inv, p_hat = R.tps_constants(62, 4, 6)                                   # F + 3 = 65 rows do not fit the kernel's LDS
    refused(tps_sample, ctx, R.tps_crops(1, 4, 6), R.tps_fiducials(62)[None], inv, p_hat)


# ---------------------------------------------------------------------------------------------------------- attention cell
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cid,kw", R.ATTN_CONTEXT_CASES, ids=[c for c, _ in R.ATTN_CONTEXT_CASES])
def test_attn_context(ctx, cid, kw, prec):
    from marie_icr_amd.icr import attn_context

    c = R.attn_context_case(**kw)
    ref = R.attn_context(c["hproj"], c["hp"][:, :256], c["score_w"], c["H"])
    out = attn_context(ctx, prec_of(prec), c["hproj"], c["hp"], c["score_w"], c["H"])
    close(f"attn_context {prec} {cid}", split(out, ref.shape, cid, prec == "f16"), ref)


@pytest.mark.parametrize("prec", PRECS)
def test_attn_context_refuses(ctx, prec):
    from marie_icr_amd.icr import attn_context

    c = R.attn_context_case(T=1, B=1, ld_hp=256, sharp=False)
    z = np.zeros((1, 65, 256), np.float32)                                      # T = 65: one score more than the LDS array holds
    refused(attn_context, ctx, prec_of(prec), z, c["hp"], c["score_w"], z)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [1, 3])
def test_attn_cell(ctx, B, prec):
    from marie_icr_amd.icr import attn_cell

    c = R.attn_cell_case(B)
    h_ref, c_ref = R.attn_cell(c["gctx"], c["ghid"][:, 256:], c["w_onehot"], c["chars"], c["c_prev"])
    c_out, h_out = attn_cell(ctx, prec_of(prec), c["gctx"], c["ghid"], c["w_onehot"], c["chars"], c["c_prev"])
    close(f"attn_cell {prec} B{B} c (in place)", split(c_out, c_ref.shape, "c"), c_ref)
    close(f"attn_cell {prec} B{B} h", split(h_out, h_ref.shape, "h", prec == "f16"), h_ref)


def test_attn_cell_entry_refuses_a_wild_character(ctx):
    from marie_icr_amd.icr import attn_cell

    c = R.attn_cell_case(1)
    for bad in (-1, R.NUM_CLASS, 0x7FFFFFFF):
        refused(attn_cell, ctx, prec_of("f32"), c["gctx"], c["ghid"], c["w_onehot"], np.array([bad], np.int32), c["c_prev"])


# ---------------------------------------------------------------------------------------------------------- arg-max
# The rows from `first_nonfinite` on (all -inf; a NaN in the last column; NaNs in columns 3 and 70) came back as 0x7fffffff before
# argmax_before() (csrc/icr_ops.hip) gave the kernels torch.max's order: they started from that index and replaced it only on
# v > best, which neither -inf nor a NaN satisfies.
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "ld4704"])
@pytest.mark.parametrize("C", R.ARGMAX_C)
def test_argmax_rows(ctx, C, wide):
    from marie_icr_amd.icr import argmax_rows

    rows, names, first_nf = R.argmax_rows_case(C)
    ld = 49 * 96 if wide else C
    x = np.full((rows.shape[0], ld), np.inf, np.float32)                    # columns >= C inside ld must be ignored
    x[:, :C] = rows
    ref = R.argmax_rows(rows, C)
    dev = split(argmax_rows(ctx, x, C), ref.shape, f"C{C}")
    print(f"argmax_rows C{C} ld{ld}: rows {names}\n  kernel {dev.tolist()}\n  torch  {ref.tolist()}")
    assert ((dev >= 0) & (dev < C)).all(), "an index outside [0, C)"
    np.testing.assert_array_equal(dev[:first_nf], ref[:first_nf])
    np.testing.assert_array_equal(dev[first_nf:], ref[first_nf:])         # the non-finite rows


def test_argmax_rows_refuses(ctx):
    from marie_icr_amd.icr import argmax_rows

    refused(argmax_rows, ctx, np.zeros((2, 8), np.float32), 9)               # ld < C
    refused(argmax_rows, ctx, np.zeros((2, 8), np.float32), 0)


@pytest.mark.parametrize("C", R.ARGMAX_C)
def test_rowmax_softmax(ctx, C):
    from marie_icr_amd.icr import rowmax_softmax

    rows, names, first_nf = R.argmax_rows_case(C)
    ref = R.argmax_rows(rows, C)
    idx, pmax = rowmax_softmax(ctx, rows)
    idx, pmax = split(idx, ref.shape, f"C{C} idx"), split(pmax, ref.shape, f"C{C} pmax")
    print(f"rowmax_softmax C{C}: rows {names}\n  kernel {idx.tolist()}\n  torch  {ref.tolist()}")
    assert ((idx >= 0) & (idx < C)).all(), "an index outside [0, C)"
    np.testing.assert_array_equal(idx, ref)
    p_ref = R.softmax_pmax(rows[:first_nf])
    rel = np.abs(pmax[:first_nf].astype(np.float64) - p_ref) / p_ref
    print(f"  pmax relative error {rel.max():.2e} (bar {R.PMAX_RTOL:.0e})")
    assert rel.max() <= R.PMAX_RTOL
    if C == 1:
        assert (pmax[:first_nf] == 1.0).all()                                 # a one-column row gives exactly 1
    assert np.isnan(pmax[first_nf:]).all()                                    # as the float64 soft-max of these rows
