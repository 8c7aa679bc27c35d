"""Kernel-level parity of conv_igemm's convolution paths with the plain epilogue — the tap gather and its zero padding, both pooled
row orders, the two-tensor input, vertical stride and asymmetric padding, the residual, pitched and periodically mapped output
rows, the `pure` pointer walk and its switch to the general gather — each alone through the C ABI (mhip_conv2d_nhwc_ex), on every
tile shape, against the float64 tap-sum reference of tests/conv_ref.py computed from the SAME rounded operands the device gets.

Every bar is derived from u16 = 2^-11 (f16 rounding), u32 = 2^-24 (fp32 rounding) and magnitudes the reference computes:
  per element   |got - ref| <= u_out |ref| + 2^-25 + (K + 4) u32 mag      (worst case of fp32 accumulation in any order; the f32 mode's
                                                                          v_mfma_f32_16x16x4_f32 rounds once per accumulation step)
  on the mean   mean|got - ref| <= mean(u_out |ref| + 2^-25 + sqrt(K) u32 mag)
                mag = |scale| conv(|in|, |w|) + |bias| + |res|,  K = KH KW Cin,  u_out = u16 for f16 outputs, u32 for fp32 outputs
  GELU          the bound of the pre-activation t times max|gelu'| <= 1.13, plus (|t| / 2) (1.5e-7 + 4 u32) for the kernel's erf
                (A&S 7.1.26) with its rcp and exp2
  ReLU, max     1-Lipschitz: the bound of a pooled output is the largest bound in its window
Each case names the kernel the launcher's rule picks for it and asserts, through the launch profile, that exactly this one ran.
Outputs are NaN-filled with GUARD sentinel rows behind them: every owned element comes out finite, everything else (guard rows,
columns beyond N of a pitched row, rows a periodic mapping skips) stays bit-untouched.  Measured error / bound ratios are written
as conv_errors.json beside the other parity reports.  The case tables are in tests/conv_cases.py."""
import math

import pytest
import torch

import conv_cases as cc
import conv_ref as cr
from test_fullsize_gpu import _report
from test_gemm_fold_gpu import GUARD, U16, U32, _guarded, _same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILES = (cc.T64, cc.T128, cc.T256, cc.S128)
POISON = 1.0e4                   # behind and beside the residual: one such value read breaks every bound
ERRORS = {}
_REFS = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def _rule(M, N, pool, dual):
    """the kernel mhip_launch_conv_igemm picks for the plain epilogue; M = the rows it enumerates (4 / 2 per pooled pixel).  Restated
    here only to keep the case tables honest: what actually ran is asserted from the launch profile."""
    bn = 256 if N > 128 else (128 if N > 64 else 64)
    mt = -(-M // (512 if bn == 64 else 256))
    if bn == 256 and mt * -(-N // 256) < 192 and mt * -(-N // 128) >= 192:
        return cc.T128
    if mt * -(-N // bn) < 192 and N > 64 and pool == cc.P0 and not dual:
        return cc.S128
    return {64: cc.T64, 128: cc.T128, 256: cc.T256}[bn]


def _case_rule(case, H=None):
    c = dict(case, H=H or case["H"])
    return _rule(cc.geometry(c)[4], c["N"], c["pool"], bool(c["Cin1"]))


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _launch(ctx, prec, desc, ptrs, expect_tile=None):
    """one mhip_conv2d_nhwc_ex call; returns after the stream has drained.  With `expect_tile`: exactly that kernel ran, once."""
    from marie_icr_amd._lib import PREC_F16, PREC_F32

    p = PREC_F16 if prec == "f16" else PREC_F32
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if expect_tile is None:
        ctx.conv2d_nhwc_ex(p, desc, *ptrs)
    else:
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            ctx.conv2d_nhwc_ex(p, desc, *ptrs)
            prof = ctx.profile_read()
        finally:
            ctx.profile_enable(False)
        ran = {k: prof[k]["launches"] for k in TILES}
        assert ran == {k: int(k == expect_tile) for k in ran}, (expect_tile, ran)
    torch.cuda.synchronize()


def _desc(c, prec, res_ptr=0):
    from marie_icr_amd._lib import ConvExDesc

    d = ConvExDesc()
    for f, v in (("B", c["B"]), ("H", c["H"]), ("W", c["W"]), ("Cin", cc.cin(c, prec)), ("KH", c["KH"]), ("KW", c["KW"]),
                 ("pad", c["pad"]), ("N", c["N"]), ("pool", c["pool"]), ("relu", c["act"]), ("out_f32", c["out_f32"]),
                 ("dil", c["dil"]), ("Cin1", c["Cin1"]), ("ldc", c["ldc"]), ("pad_cols_writable", c["own"]), ("sy", c["sy"]),
                 ("pad_x", c["pad_x"]), ("row_period", c["period"]), ("row_stride", c["row_stride"]), ("row_offset", c["row_offset"])):
        setattr(d, f, int(v))
    d.res_dev = res_ptr or None
    return d


def _out_dtype(c, prec):
    return torch.float32 if (c["out_f32"] or prec == "f32") else torch.float16


def _residual_on_device(c, res, ld):
    """the residual's R rows at the output's pitch, GUARD rows of POISON behind them and POISON in the columns beyond N, at
    `res_shift` bytes off a 16-byte boundary -> (device view [R + GUARD][ld], the flat tensor that owns the memory)"""
    R, N = res.shape
    shift = c["res_shift"] // res.element_size()
    host = torch.full(((R + GUARD) * ld + 16,), POISON, dtype=res.dtype)
    view = host[shift:shift + (R + GUARD) * ld].view(R + GUARD, ld)
    view[:R, :N] = res
    flat = host.to(DEV)
    dview = flat[shift:shift + (R + GUARD) * ld].view(R + GUARD, ld)
    assert dview.data_ptr() % 16 == c["res_shift"] % 16
    return dview, flat


def _run(ctx, case, prec, ops, H=None):
    """launch the case (on a map of H rows if given) -> the owned output [B][Hp][Wp][N] on the host, after checking which kernel
    ran, that every owned element was written and that nothing else was"""
    c = dict(case, H=H or case["H"])
    _, _, Hp, Wp, _, rows = cc.geometry(c)
    N, ld = c["N"], c["ldc"] or c["N"]
    brow = cr.out_rows(rows, c["period"], c["row_stride"], c["row_offset"])
    buf_rows = (rows // c["period"]) * c["row_stride"] + c["row_offset"] if c["period"] else rows
    assert int(brow.max()) < buf_rows
    out = _guarded(buf_rows, ld, _out_dtype(c, prec), 7.0)
    before = out.clone()
    dev = {k: (None if v is None else v.to(DEV)) for k, v in ops.items() if k != "res"}
    res_view = keep = None
    if ops["res"] is not None:
        res_view, keep = _residual_on_device(c, ops["res"], ld)
    ptr = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    _launch(ctx, prec, _desc(c, prec, ptr(res_view)),
            (ptr(dev["x"]), ptr(dev["w"]), ptr(dev["scale"]), ptr(dev["bias"]), out.data_ptr(), ptr(dev["x2"])), c["tile"])
    del keep
    assert _same_bits(out[buf_rows:], before[buf_rows:]), f"{c['name']}: guard rows behind the output were written"
    own = cr.owned(buf_rows + GUARD, ld, brow, N, bool(c["own"])).to(DEV)
    assert _same_bits(out[~own], before[~own]), f"{c['name']}: elements the call does not own were written"
    brow_d = brow.to(DEV)
    got = out[brow_d, :N]
    assert bool(torch.isfinite(got).all()), f"{c['name']}: unwritten or non-finite output elements"
    if c["own"]:
        assert bool((out[brow_d, N:(N + 7) // 8 * 8] == 0).all()), f"{c['name']}: the call's own pad columns are not zeros"
    return got.cpu().view(c["B"], Hp, Wp, N)


def _reference(case, prec):
    """operands and float64 reference of a case, made once per module and left unchanged"""
    key = (case["name"], prec)
    if key not in _REFS:
        ops = cc.operands(case, prec)
        r = cr.conv_ref(ops["x"], ops["w"], x2=ops["x2"], scale=ops["scale"], bias=ops["bias"], sy=case["sy"], pad=case["pad"],
                        pad_x=case["pad_x"], dil=case["dil"], act=case["act"], res=ops["res"], pool=case["pool"],
                        row_period=case["period"])
        _REFS[key] = (ops, r)
    return _REFS[key]


def _bounds(case, prec, r):
    """-> the per-element bound and the mean form, at the shape of the (pooled) output"""
    K = case["KH"] * case["KW"] * cc.cin(case, prec)
    u_out = U32 if _out_dtype(case, prec) == torch.float32 else U16
    if case["act"] == cc.GELU:
        k, extra = 1.13, (r["t"].abs() / 2) * (1.5e-7 + 4 * U32)
    else:
        k, extra = 1.0, 0.0
    base = u_out * r["v"].abs() + 2.0 ** -25 + extra
    hard, meanb = base + k * (K + 4) * U32 * r["mag"], base + k * math.sqrt(K) * U32 * r["mag"]
    return cr.pool_max(hard, case["pool"]), cr.pool_max(meanb, case["pool"])


def _check(tag, group, got, ref, hard, meanb):
    err = (got.double() - ref).abs()
    rec = {"group": group, "max_err_over_bound": float((err / hard).max()), "mean_err_over_mean_bound": float(err.mean() / meanb.mean())}
    _report(tag, rec, ERRORS, "conv_errors.json")
    print(f"{tag}: max err/bound {rec['max_err_over_bound']:.3f}  mean err / mean bound {rec['mean_err_over_mean_bound']:.3f}")
    bad = torch.nonzero(err > hard)
    assert bad.numel() == 0, (tag, "first element over the hard bound", bad[0].tolist(), float(err[tuple(bad[0])]), float(hard[tuple(bad[0])]))
    assert err.mean() <= meanb.mean(), (tag, "mean error over the mean bound", rec)


# ---------------------------------------------------------------------------------------------------------------------- parity
PARITY = [(g, c, p) for g, cases in cc.GROUPS.items() for c in cases for p in c["precs"]]


@pytest.mark.parametrize("group,case,prec", PARITY, ids=[f"{c['name']}/{p}" for _, c, p in PARITY])
def test_conv_path(ctx, group, case, prec):
    """one case of tests/conv_cases.py: the kernel that ran, the owned and the untouched elements, and every element against float64.
    (Both precisions run every case, the 49 087-pixel maps included: their float64 references are some 20 GFLOP each, seconds.)"""
    assert _case_rule(case) == case["tile"]
    ops, r = _reference(case, prec)
    if group == "residual":        # a ReLU applied before the add instead of after it must show
        res = ops["res"].double().reshape(r["t"].shape)
        up, down = (r["t"] < 0) & (r["t"] + res > 0), (r["t"] > 0) & (r["t"] + res < 0)
        assert float(up.double().mean()) >= 0.05 and float(down.double().mean()) >= 0.05
    if case["neg"]:                # a max that starts from zero must show: most windows are negative throughout
        assert float((r["out"] < 0).double().mean()) >= 0.5
    got = _run(ctx, case, prec, ops)
    hard, meanb = _bounds(case, prec, r)
    _check(f"{case['name']}/{prec}", group, got, r["out"], hard, meanb)


# ------------------------------------------------------------------------------- straight-line and bounds-checked copies agree
@pytest.mark.parametrize("N,W,H,tile,bm", cc.PAIRS)
def test_straight_line_and_bounds_checked_conv_f16_agree(ctx, N, W, H, tile, bm):
    """the unpooled 3x3 conv into f16 on maps of H, H - 1 and H + 1 rows of the same operands: the output rows whose taps see the
    same pixels in two runs are the same bits.  Against the shorter map this sets `f16_fast` against `body` (see conv_cases.PAIRS)."""
    case = cc.pair_case(N, W, H, tile)
    assert all(_case_rule(case, h) == tile for h in (H - 1, H, H + 1))
    Ms, shared = (H - 1) * W, (H - 2) * W                  # the shorter map's pixels; those whose taps reach no missing row
    assert Ms % bm > Ms - shared and Ms // bm < (H * W) // bm, "no shared row lies in a tile that one run fills and the other does not"
    ops = cc.operands(case, "f16", H=H + 1)
    outs = {h: _run(ctx, case, "f16", dict(ops, x=ops["x"][:, :h].contiguous()), H=h) for h in (H, H - 1, H + 1)}
    assert _same_bits(outs[H][:, :H - 2], outs[H - 1][:, :H - 2]), f"rows shared by H = {H} and H = {H - 1} differ"
    assert _same_bits(outs[H][:, :H - 1], outs[H + 1][:, :H - 1]), f"rows shared by H = {H} and H = {H + 1} differ"
    # ... and the rows that are NOT shared differ: the comparison above is not between copies of one buffer
    assert not _same_bits(outs[H][:, H - 2:H - 1], outs[H - 1][:, H - 2:H - 1])


def test_every_plain_instantiation_is_cased():
    """each case asserts the kernel that ran; this keeps the tables covering all 26 instantiations of the plain epilogue:
    {f16, f32} x ({64, 128, 256} x {unpooled, 2x2, 2x1, two inputs} + the 128 x 128 tile)"""
    kind = lambda c: "dual" if c["Cin1"] else {cc.P0: "none", cc.P22: "2x2", cc.P21: "2x1"}[c["pool"]]      # noqa: E731
    have = {(p, c["tile"], kind(c)) for c in cc.ALL for p in c["precs"]}
    want = {(p, t, k) for p in ("f16", "f32") for t in (cc.T64, cc.T128, cc.T256) for k in ("none", "2x2", "2x1", "dual")}
    want |= {(p, cc.S128, "none") for p in ("f16", "f32")}
    assert have == want and len(want) == 26
    assert {t for _, _, _, t, _ in cc.PAIRS} == set(TILES)
    # the unpooled 3x3 convolution itself (not only a 1x1 GEMM) runs on each of the four shapes
    assert {c["tile"] for c in cc.ALL if c["KH"] == 3 and c["pool"] == cc.P0 and c["dil"] == 1} == set(TILES)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    """every documented refusal of the launcher comes back as an error through the new entry, and nothing is written"""
    from marie_icr_amd._lib import MarieHipError

    base = cc._c("refuse/base", cc.S128, H=6, W=11, act=cc.RELU)
    x = torch.zeros((2, 6, 11, 256), dtype=torch.float16).to(DEV)
    w = torch.zeros((256, 3, 3, 256), dtype=torch.float16).to(DEV)
    out = torch.zeros((4 * 132 + GUARD, 256), dtype=torch.float16).to(DEV)
    res = torch.zeros((4 * 132 + GUARD, 256), dtype=torch.float16).to(DEV)

    def call(c, with_res=False, with_x2=False):
        _launch(ctx, "f16", _desc(c, "f16", res.data_ptr() if with_res else 0),
                (x.data_ptr(), w.data_ptr(), 0, 0, out.data_ptr(), x.data_ptr() if with_x2 else 0))

    gemm = dict(base, B=1, H=1, W=150, KH=1, KW=1, pad=0)
    cat = dict(base, KH=1, KW=1, pad=0, Cin=128, Cin1=64)
    for c, kw in ((base, {}), (base, dict(with_res=True)), (dict(gemm, period=50, row_stride=53, row_offset=1), dict(with_res=True)),
                  (cat, dict(with_x2=True)), (dict(base, ldc=136), {})):            # the bases themselves are accepted
        call(c, **kw)
    out.zero_()
    bad = [
        ("residual with a pooled output", dict(base, pool=cc.P22), dict(with_res=True)),
        ("residual with a 2x1-pooled output", dict(base, pool=cc.P21), dict(with_res=True)),
        ("GELU with a residual", dict(base, act=cc.GELU), dict(with_res=True)),
        ("row mapping with pooling", dict(base, period=4, row_stride=4, pool=cc.P22), {}),
        ("row_stride < row_period", dict(gemm, period=50, row_stride=49), {}),
        ("pitched row not 16-byte aligned", dict(base, ldc=132), {}),
        ("pitch below N", dict(base, ldc=120), {}),
        ("pitched pooled output", dict(base, ldc=136, pool=cc.P22), {}),
        ("residual row not 16-byte aligned", dict(base, N=44), dict(with_res=True)),
        ("Cin1 not on a slice boundary", dict(cat, Cin1=32), dict(with_x2=True)),
        ("Cin1 = Cin", dict(cat, Cin1=128), dict(with_x2=True)),
        ("two inputs under a 3x3 filter", dict(cat, KH=3, KW=3, pad=1), dict(with_x2=True)),
        ("Cin not a whole number of slices", dict(base, Cin=96), {}),
        ("empty output", dict(base, H=1, KH=2, KW=2, pad=0), {}),
        ("negative stride", dict(base, sy=-1), {}),
        ("pad_x below -1", dict(base, pad_x=-2), {}),
    ]
    for what, c, kw in bad:
        with pytest.raises(MarieHipError):
            call(c, **kw)
            pytest.fail(f"accepted: {what}")
    torch.cuda.synchronize()
    assert bool((out == 0).all()), "a refused call wrote output"
