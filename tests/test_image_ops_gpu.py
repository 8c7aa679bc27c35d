"""Kernel-level parity of the detector's image kernels (csrc/image_ops.hip), each alone through its stage entry (mhip_*_host ->
the launcher the CRAFT model calls) against the float64 statements of tests/icr_ops_ref.py.

Bars: the max-pools and the 8-bit resize bitwise; fp32 mode max |kernel - fp64| <= 1e-3 on outputs the CPU test
asserts to be O(1); 1e-3 too for the f16 up-sampling, whose only f16 step is the rounding of an output <= 2; for the two f16
kernels that round operands inside (conv_rgb_first_mfma: pixels and filters; score_head: the hidden activation)
max |kernel - fp64| <= 2 * E_ref, E_ref = max |f16-emulated float64 - float64| computed here with the same rounding points.
tests/test_icr_ops_ref_cpu.py shows without a GPU that each mistake named there moves the reference by at least 50 bars on
exactly these inputs."""
import numpy as np
import pytest

import icr_ops_ref as R
from test_icr_ops_gpu import close, prec_of, refused, split

pytestmark = pytest.mark.gpu
PRECS = ["f16", "f32"]


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _by_prec(cases):
    """(case..., precisions) -> one parameter set per precision"""
    out = [c[:-1] + (p,) for c in cases for p in c[-1]]
    return out, [f"{c[0]}-{c[-1]}" for c in out]


# ---------------------------------------------------------------------------------------------------------- conv_rgb_first
# MI355X, first run (f16: the MFMA kernel, bar 2 * E_ref):
#   th x tw on H x W      E_ref      f16 err    fp32 err
#   3 x 5                 4.91e-04   4.91e-04   1.58e-07
#   17 x 23               7.80e-04   7.80e-04   2.17e-07
#   30 x 45 on 32 x 64    6.65e-04   6.65e-04   3.26e-07
#   520 x 512             7.02e-04   7.02e-04   4.68e-07
# The f16 kernel's error equals the emulation's to three digits: both are the half-ulp rounding of an output in [1, 2).
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("th,tw,H,W", R.RGB_SHAPES, ids=str)
def test_conv_rgb_first(ctx, th, tw, H, W, prec):
    from marie_icr_amd.craft import conv_rgb_first

    c = R.rgb_case(th, tw, H, W)
    args = (c["img"], H, W, c["w"], c["scale"], c["bias"])
    ref = R.conv_rgb_first(*args)
    dev = split(conv_rgb_first(ctx, prec_of(prec), *args), ref.shape, f"{th}x{tw}", prec == "f16")
    tag = f"conv_rgb_first {prec} {th}x{tw} on {H}x{W}"
    if prec == "f16":
        e_ref = float(np.abs(R.conv_rgb_first(*args, f16_emulated=True) - ref).max())
        print(f"{tag}: E_ref {e_ref:.2e}")
        close(tag, dev, ref, 2 * e_ref)
    else:
        close(tag, dev, ref)


@pytest.mark.parametrize("prec", PRECS)
def test_conv_rgb_first_refuses(ctx, prec):
    from marie_icr_amd.craft import conv_rgb_first

    c = R.rgb_case(3, 5, 3, 5)
    refused(conv_rgb_first, ctx, prec_of(prec), c["img"], 3, 4, c["w"], c["scale"], c["bias"])      # tw > W


# ---------------------------------------------------------------------------------------------------------- max-pools
MAXPOOL, MAXPOOL_IDS = _by_prec(R.MAXPOOL_CASES)


@pytest.mark.parametrize("cid,k,shape,neg,prec", MAXPOOL, ids=MAXPOOL_IDS)
def test_maxpool(ctx, cid, k, shape, neg, prec):
    from marie_icr_amd.craft import maxpool

    x = R.pool_input(67, shape, neg)
    ref = R.maxpool(x, k).astype(np.float32)
    dev = split(maxpool(ctx, prec_of(prec), k, x), ref.shape, cid, prec == "f16")
    diff = int((dev.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"maxpool {prec} {cid}: {diff} of {ref.size} outputs differ")
    assert diff == 0


@pytest.mark.parametrize("prec", PRECS)
def test_maxpool_refuses(ctx, prec):
    from marie_icr_amd.craft import maxpool

    refused(maxpool, ctx, prec_of(prec), 4, np.zeros((1, 4, 4, 8), np.float32))             # K = 4
    refused(maxpool, ctx, prec_of(prec), 2, np.zeros((1, 4, 4, 6), np.float32))             # C = 6: no whole vector


# ---------------------------------------------------------------------------------------------------------- up-sampling
UPSAMPLE, UPSAMPLE_IDS = _by_prec(R.UPSAMPLE_CASES)


@pytest.mark.parametrize("cid,shape,size,prec", UPSAMPLE, ids=UPSAMPLE_IDS)
def test_upsample_bilinear(ctx, cid, shape, size, prec):
    from marie_icr_amd.craft import upsample_bilinear

    x = R.upsample_input(73, shape)
    ref = R.upsample_bilinear(x, *size)
    dev = split(upsample_bilinear(ctx, prec_of(prec), x, *size), ref.shape, cid, prec == "f16")
    close(f"upsample_bilinear {prec} {cid}", dev, ref)


# ---------------------------------------------------------------------------------------------------------- score head
# MI355X, first run (f16 bar 2 * E_ref):
#   case                  E_ref      f16 err    fp32 err
#   stride16-n1           1.26e-04   1.26e-04   5.92e-08
#   stride64-n1           1.11e-04   1.11e-04   7.79e-08
#   stride16-n257         4.16e-04   4.16e-04   2.57e-07
#   stride64-n257         6.18e-04   6.18e-04   3.29e-07
#   stride16-n2100000     5.94e-04   5.94e-04   (f16 only)
SCORE, SCORE_IDS = _by_prec(R.SCORE_CASES)


@pytest.mark.parametrize("cid,stride,npix,prec", SCORE, ids=SCORE_IDS)
def test_score_head(ctx, cid, stride, npix, prec):
    from marie_icr_amd.craft import score_head

    c = R.score_case(stride, npix)
    args = (c["x"][:, :16], c["w1"], c["b1"], c["w2"], c["b2"])
    ref = R.score_head(*args)
    dev = split(score_head(ctx, prec_of(prec), c["x"], *args[1:]), ref.shape, cid)
    tag = f"score_head {prec} {cid}"
    if prec == "f16":
        e_ref = float(np.abs(R.score_head(*args, f16_emulated=True) - ref).max())
        print(f"{tag}: E_ref {e_ref:.2e}")
        close(tag, dev, ref, 2 * e_ref)
    else:
        close(tag, dev, ref)


# ---------------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("src,dst", R.RESIZE_CASES, ids=str)
def test_resize_linear_u8(ctx, src, dst):
    from marie_icr_amd.craft import resize_linear_u8

    img = np.random.default_rng(79).integers(0, 256, size=src + (3,)).astype(np.uint8)
    ref = R.resize_linear_u8(img, *dst)
    out = resize_linear_u8(ctx, img, *dst)
    n = ref.size
    assert (out[n:] == 255).all(), "the guard behind the output was written"
    diff = int((out[:n].reshape(ref.shape) != ref).sum())
    print(f"resize_linear_u8 {src} -> {dst}: {diff} of {n} bytes differ")
    assert diff == 0
