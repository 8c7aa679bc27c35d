"""The row LayerNorm every tower shares (marie_icr_amd/csrc/row_ops.hip: row_layernorm_kernel, arithmetic in row_ops.h), alone
through its stage entry mhip_row_layernorm_host against the float64 layer_norm of tests/bert_text_ref.py.

Shapes: D 64 (one partly filled float4 group per lane), 192 (no multiple of 256), 256 (exactly one group), 320 (one full group and
a partial one), 768 (three), 1024 (four); rows 1 (a single wave) and 5 (a second workgroup whose last three waves have no row).
Forms: fp32 in with both outputs; the element-type output alone (h null: the CLIP towers); in place (h == x: the TrOCR decoder);
and, in the f16 mode, the f16 stream without and with a low plane (the ViT; the plane here is of order 1, not a rounding residue, so
that dropping it would miss every bar).
Inputs: standard-normal rows, one row of mean 100 and deviation 1, one constant row; g = 1 + 0.3 N, b = 0.2 N; eps 1e-5 and 1e-12.

Bars:
  * fp32 output: 1e-3 absolute, the bar test_berttext_gpu.py::test_embed_kernel holds the same arithmetic to;
  * f16 output: max |kernel - fp64| <= 2 E_ref with E_ref = max |r16(fp64) - fp64|, the form of test_geglu_kernel;
  * the constant row returns b exactly in fp32 (mean exact, every difference 0);
  * the three fp32-in forms are bit-equal to one another; in the fp32 mode the element-type output is the fp32 output;
  * every output's STAGE_GUARD elements still hold the 0xff fill, and every cell in front of them was written.
Every case prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16 = 1, 0
WIDTHS = [64, 192, 256, 320, 768, 1024]
EPS = [1e-5, 1e-12]
CONST = 2.5                      # exact in f16; its sums up to 1024 columns and their mean are exact in fp32
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emb_mod():
    from marie_icr_amd import embeddings

    return embeddings


def _inputs(D):
    """x fp32 (5, D): normal, mean 100 / deviation 1, constant, normal, normal; g, b fp32 (D); computed once, left unchanged"""
    if ("in", D) not in _cache:
        rng = np.random.default_rng(D)
        x = rng.standard_normal((5, D))
        x[1] += 100.0
        x[2] = CONST
        g, b = 1 + 0.3 * rng.standard_normal(D), 0.2 * rng.standard_normal(D)
        arrs = tuple(np.ascontiguousarray(a, np.float32) for a in (x, g, b))
        for a in arrs:
            a.setflags(write=False)
        _cache[("in", D)] = arrs
    return _cache[("in", D)]


def _want(key, x, g, b, eps):
    """float64 LayerNorm of fp32 / f16-representable inputs, computed once per key"""
    if key not in _cache:
        w = R.layer_norm(np.asarray(x, np.float64), g.astype(np.float64), b.astype(np.float64), eps)
        w.setflags(write=False)
        _cache[key] = w
    return _cache[key]


def _split(out, shape, tag, widened_f16=False):
    """the output proper, after checking the guard behind it and that every cell in front was written"""
    from marie_icr_amd._lib import STAGE_GUARD

    n = int(np.prod(shape))
    assert out.size == n + STAGE_GUARD
    fill = np.uint32(0xFFFFE000 if widened_f16 else 0xFFFFFFFF)          # f16 0xffff widens to this fp32 NaN
    assert (out[n:].view(np.uint32) == fill).all(), f"{tag}: the guard behind the output was written"
    assert np.isfinite(out[:n]).all(), f"{tag}: unwritten or non-finite cells"
    return out[:n].reshape(shape)


def _check(tag, precision, h, ht, want, b, const_rows):
    """h (fp32, or None) and ht (element type, widened) against the float64 rows"""
    if h is not None:
        err = np.abs(h - want).max()
        print(f"{tag}: fp32 max |d| {err:.3e} (entries up to {np.abs(want).max():.2f})")
        assert err <= 1e-3
        for r in const_rows:
            assert np.array_equal(h[r], b), f"{tag}: the constant row is not b"
    if precision == F32:
        err = np.abs(ht - want).max()
        print(f"{tag}: element-type (fp32) max |d| {err:.3e}")
        assert err <= 1e-3
        if h is not None:
            assert np.array_equal(h, ht), f"{tag}: the fp32 mode's two outputs differ"
    else:
        err, e_ref = np.abs(ht - want).max(), np.abs(R.r16(want) - want).max()
        print(f"{tag}: f16 max |d| {err:.3e}, E_ref {e_ref:.3e}")
        assert err <= 2 * e_ref


def _row_sets(rows):
    """(first row, constant rows) of the calls of a case: all five rows at once, or each kind of row alone"""
    return [(0, [2])] if rows == 5 else [(0, []), (1, []), (2, [0])]


@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", WIDTHS)
def test_fp32_rows(ctx, emb_mod, D, rows, precision):
    x5, g, b = _inputs(D)
    f16 = precision == F16
    for eps in EPS:
        for r0, const_rows in _row_sets(rows):
            x = x5[r0:r0 + rows]
            want = _want(("f32", D, eps), x5, g, b, eps)[r0:r0 + rows]
            tag = f"row_layernorm {'f16' if f16 else 'f32'} D {D} rows {rows} (from {r0}) eps {eps:g}"
            h, ht = emb_mod.row_layernorm_host(ctx, precision, x, g, b, eps)
            h, ht = _split(h, x.shape, tag + " h"), _split(ht, x.shape, tag + " ht", f16)
            _check(tag, precision, h, ht, want, b, const_rows)
            none, only = emb_mod.row_layernorm_host(ctx, precision, x, g, b, eps, want_h=False)
            assert none is None
            assert np.array_equal(_split(only, x.shape, tag + " ht alone", f16), ht), f"{tag}: ht alone differs"
            hp, tp = emb_mod.row_layernorm_host(ctx, precision, x, g, b, eps, in_place=True)
            assert np.array_equal(_split(hp, x.shape, tag + " in place h"), h), f"{tag}: in place differs"
            assert np.array_equal(_split(tp, x.shape, tag + " in place ht", f16), ht), f"{tag}: in place differs"


@pytest.mark.parametrize("with_lo", [False, True], ids=["hi", "hi+lo"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", WIDTHS)
def test_f16_stream(ctx, emb_mod, D, rows, with_lo):
    x5, g, b = _inputs(D)
    hi5 = R.r16(x5)
    lo5 = None
    if with_lo:      # a low plane of order 1, so that a kernel that dropped it misses every bar; hi + lo is exact in fp32
        lo5 = R.r16(0.75 * np.random.default_rng(D + 1).standard_normal(x5.shape))
        lo5[2] = 0.25                                               # the constant row stays constant
    for eps in EPS:
        want5 = _want(("f16", D, eps, with_lo), hi5 + (lo5 if with_lo else 0.0), g, b, eps)
        for r0, const_rows in _row_sets(rows):
            sl = slice(r0, r0 + rows)
            tag = f"row_layernorm f16 stream{' + low plane' if with_lo else ''} D {D} rows {rows} (from {r0}) eps {eps:g}"
            h, ht = emb_mod.row_layernorm_host(ctx, F16, hi5[sl], g, b, eps, x_f16=True, x_lo=lo5[sl] if with_lo else None)
            shape = (rows, D)
            h, ht = _split(h, shape, tag + " h"), _split(ht, shape, tag + " ht", True)
            _check(tag, F16, h, ht, want5[sl], b, const_rows)
            none, only = emb_mod.row_layernorm_host(ctx, F16, hi5[sl], g, b, eps, want_h=False, x_f16=True,
                                                    x_lo=lo5[sl] if with_lo else None)
            assert none is None
            assert np.array_equal(_split(only, shape, tag + " ht alone", True), ht), f"{tag}: ht alone differs"


def test_refusals(ctx, emb_mod):
    from marie_icr_amd._lib import MarieHipError

    x, g, b = _inputs(64)
    for bad in (dict(precision=F32, x_f16=True),                                   # an f16 stream needs the f16 mode
                dict(precision=F16, x_lo=np.zeros_like(x)),                        # a low plane needs a high plane
                dict(precision=F16, want_h=False, want_ht=False)):                 # nothing to write
        with pytest.raises(MarieHipError):
            emb_mod.row_layernorm_host(ctx, bad.pop("precision"), x, g, b, 1e-5, **bad)
    with pytest.raises(MarieHipError):                                             # a width that is no multiple of 64
        emb_mod.row_layernorm_host(ctx, F32, x[:, :32], g[:32], b[:32], 1e-5)
