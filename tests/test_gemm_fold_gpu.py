"""Kernel-level parity of conv_igemm's LayerNorm-folded epilogues (EPI_SPLIT, EPI_LN_ROWS, EPI_LN_COLS), of ln_finalize and of
token_init_split, each alone through the C ABI (mhip_gemm_ln_fold, mhip_ln_finalize, mhip_token_init_split), against float64 on
the CPU computed from the SAME f16-rounded operands the device gets.

Every bar is derived from u16 = 2^-11 (f16 rounding), u32 = 2^-24 (fp32 rounding) and magnitudes the reference computes:
  consumers   |got - ref| <= u16 |ref| + 2^-25 + (K + 4) u32 mag   per element   (worst case of fp32 accumulation in any order)
              mean|got - ref| <= mean(u16 |ref| + 2^-25 + sqrt(K) u32 mag)       (the probabilistic accumulation bound)
              mag = |rstd| (|A| |W|^T) + |mur cs| + |bias|;  GELU: the bound of the pre-activation t times max|gelu'| <= 1.13,
              plus (|t| / 2) (1.5e-7 + 4 u32) for the kernel's erf (A&S 7.1.26) with its rcp and exp2
  split       |hi + lo - x| <= 2^-21 |x| + (K + 6) u32 mag, the same mean form;  |lo| <= ulp(hi) / 2 and f16(hi + lo) == hi exactly;
              statistics to the first-order propagation of those errors;  everything the call does not own stays bit-untouched
Each case names the tile shape the launcher's rule picks for it and asserts, through the launch profile, that this shape ran.
Measured error / bound ratios are written as gemm_fold_errors.json beside the other parity reports (test_fullsize_gpu._report)."""
import math

import pytest
import torch

from test_fullsize_gpu import _report

pytestmark = pytest.mark.gpu

DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
GUARD = 256                      # sentinel rows behind every output buffer
EPS = 1e-6
NONE, GELU = 0, 2
T256, T128, S128 = "conv_igemm<256>", "conv_igemm<128>", "conv_igemm<1128>"
TILE_BM = {T256: 256, T128: 256, S128: 128}
ERRORS = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _guarded(rows, cols, dtype, sentinel):
    """[rows + GUARD][cols] on the device: NaN where the call may write, `sentinel` in the guard rows"""
    t = torch.full((rows + GUARD, cols), float("nan"), dtype=dtype)
    t[rows:] = sentinel
    return t.to(DEV)


def _launch(ctx, expect_tile=None, **kw):
    """one mhip_gemm_ln_fold call; the tensors in kw are device tensors.  Returns after the stream has drained."""
    from marie_icr_amd._lib import PREC_F16, GemmFoldDesc

    d = GemmFoldDesc()
    for name in ("in", "w", "scale", "bias", "out", "ln_a", "ln_b", "ln_cs", "row_bias", "out2", "res", "res2", "stats"):
        setattr(d, name + "_dev", _ptr(kw.get(name)) or None)
    for name in ("epi", "M", "N", "K", "act", "stats_ld", "row_period", "row_stride", "row_offset"):
        setattr(d, name, int(kw.get(name, 0)))
    prec = kw.get("precision", PREC_F16)
    if DEV == "cuda":
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if expect_tile is None:
        ctx.gemm_ln_fold(prec, d)
    else:
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            ctx.gemm_ln_fold(prec, d)
            prof = ctx.profile_read()
        finally:
            ctx.profile_enable(False)
        ran = {k: prof[k]["launches"] for k in (T256, T128, S128)}
        assert ran == {k: int(k == expect_tile) for k in ran}, (expect_tile, ran)
    if DEV == "cuda":
        torch.cuda.synchronize()


def _dump(tag):
    _report(tag, ERRORS[tag], ERRORS, "gemm_fold_errors.json")


def _record(tag, err, hard, mean_bound):
    r = {"max_err_over_bound": float((err / hard).max()), "mean_err_over_mean_bound": float(err.mean() / mean_bound.mean())}
    ERRORS[tag] = r
    _dump(tag)
    print(f"{tag}: max err/bound {r['max_err_over_bound']:.3f}  mean err / mean bound {r['mean_err_over_mean_bound']:.3f}")
    return r


def _rule(M, N):
    """the tile shape mhip_launch_conv_igemm picks for a LayerNorm-folded GEMM (restated here only to keep the case tables honest:
    what actually ran is asserted from the launch profile)"""
    mt = -(-M // 256)
    if N > 128:
        if mt * -(-N // 256) >= 192:
            return T256
        return T128 if mt * -(-N // 128) >= 192 else S128
    return T128 if mt >= 192 else S128


# ------------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _noise(g, *shape):
    return torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1


def _weights(g, N, K):
    return (_noise(g, N, K) * math.sqrt(3.0 / K)).half()


BIG_MEAN_EVERY, CONST_EVERY, OUTLIER_COLS = 37, 53, (5, 130, 701)


def _tokens(g, R, D, teeth=True):
    """[R][D] fp32 token rows as a residual stream has them: uniform noise, and with `teeth`
       (a) rows r % 37 == 5 with |mean| >= 100 std,  (b) columns 5, 130, 701 (those below D) scaled by 300 — inside f16 range —
       (c) rows r % 53 == 7 constant (variance 0)"""
    x = _noise(g, R, D)
    if teeth:
        for c in OUTLIER_COLS:
            if c < D:
                x[:, c] *= 300.0
        x[5::BIG_MEAN_EVERY] = 60.0 + 0.2 * _noise(g, len(range(5, R, BIG_MEAN_EVERY)), D)
        x[7::CONST_EVERY] = 1.5
    return x


def _ln_stats(x64):
    mean = x64.mean(1)
    var = ((x64 - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(EPS, dtype=torch.float32)))
    return mean, var, rstd


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.special.erf(t * math.sqrt(0.5)))


# ---------------------------------------------------------------------------------------------------------------- consumers
def _consumer_bounds(A16, W16, la, lb, cs, bias, act, cols, K):
    """fp64 reference of a consumer and its two bounds.  rows: la / lb indexed by m, cs / bias by n;  cols: la / lb by n, cs / bias by m"""
    A, W = A16.double(), W16.double()
    acc = A @ W.T
    mag = A.abs() @ W.abs().T
    la, lb, cs, bias = la.double(), lb.double(), cs.double(), bias.double()
    if cols:
        t = la[None, :] * acc - lb[None, :] * cs[:, None] + bias[:, None]
        mag = la.abs()[None, :] * mag + (lb[None, :] * cs[:, None]).abs() + bias.abs()[:, None]
    else:
        t = la[:, None] * acc - lb[:, None] * cs[None, :] + bias[None, :]
        mag = la.abs()[:, None] * mag + (lb[:, None] * cs[None, :]).abs() + bias.abs()[None, :]
    del acc
    if act == GELU:
        ref = _gelu64(t)
        extra = (t.abs() / 2) * (1.5e-7 + 4 * U32)
        k = 1.13
    else:
        ref, extra, k = t, 0.0, 1.0
    base = U16 * ref.abs() + 2.0 ** -25 + extra
    return ref, base + k * (K + 4) * U32 * mag, base + k * math.sqrt(K) * U32 * mag


def _plain(R):
    """the rows of `_tokens` without a large mean or zero variance (whose bounds would dominate a mean over all rows)"""
    m = torch.ones(R, dtype=torch.bool)
    m[5::BIG_MEAN_EVERY] = False
    m[7::CONST_EVERY] = False
    return m


def _check_consumer(tag, got, ref, hard, meanb, plain=None):
    """`plain`: a selection of tokens over which the mean form is asserted as well (besides the mean over the whole output)"""
    assert bool(torch.isfinite(got).all()), f"{tag}: unwritten or non-finite output elements"
    err = (got.double() - ref).abs()
    r = _record(tag, err, hard, meanb)
    if plain is not None and bool((plain[-1] if isinstance(plain, tuple) else plain).any()):
        r["plain_tokens_mean_err_over_mean_bound"] = float(err[plain].mean() / meanb[plain].mean())
        _dump(tag)
        print(f"{tag}: plain tokens alone, mean err / mean bound {r['plain_tokens_mean_err_over_mean_bound']:.3f}")
        assert r["plain_tokens_mean_err_over_mean_bound"] <= 1, (tag, "mean error over the mean bound on the plain tokens", r)
    bad = torch.nonzero(err > hard)
    assert bad.numel() == 0, (tag, "first element over the hard bound", bad[0].tolist(), float(err[tuple(bad[0])]), float(hard[tuple(bad[0])]))
    assert err.mean() <= meanb.mean(), (tag, "mean error over the mean bound", r)


def _rows_operands(seed, M, N, K, teeth=True):
    g = _gen(seed)
    A16 = _tokens(g, M, K, teeth).half()
    W16 = _weights(g, N, K)
    mean, _, rstd = _ln_stats(A16.double())
    la, lb = rstd.float(), (mean * rstd).float()
    cs = W16.double().sum(1).float()
    bias = _noise(g, N) * 0.5
    return A16, W16, la, lb, cs, bias


def _run_rows(ctx, A16, W16, la, lb, cs, bias, act, tile):
    M, K = A16.shape
    N = W16.shape[0]
    dev = [t.to(DEV) for t in (A16, W16, la, lb, cs, bias)]
    out = _guarded(M, N, torch.float16, 7.0)
    before = out.clone()
    _launch(ctx, tile, epi=1, M=M, N=N, K=K, act=act, out=out, **dict(zip(("in", "w", "ln_a", "ln_b", "ln_cs", "bias"), dev)))
    assert _same_bits(out[M:], before[M:]), "guard rows behind the output were written"
    return out[:M].cpu()


ROWS_CASES = [
    # N, K, act, M, tile            M = 4, 8, 252 (mod 256): the last row of tiles runs `body`, all others `f16_fast`
    (1536, 768, NONE, 8196, T256), (1536, 768, NONE, 4104, T128), (1536, 768, NONE, 1276, S128),      # q|k
    (3072, 768, GELU, 4348, T256), (3072, 768, GELU, 2052, T128), (3072, 768, GELU, 520, S128),       # fc1
    (1536, 768, NONE, 100, S128),                                                                       # M < 128
    (200, 768, NONE, 520, S128), (328, 768, GELU, 520, S128),                                           # partial n-tile
    (200, 768, GELU, 24580, T128), (328, 768, NONE, 24580, T256),                                       # ... on the big tiles
]


@pytest.mark.parametrize("N,K,act,M,tile", ROWS_CASES)
def test_ln_rows(ctx, N, K, act, M, tile):
    """EPI_LN_ROWS: out = act(rstd[m] acc - mur[m] cs[n] + bias[n]) with the LayerNorm statistics of the operand rows themselves
    (large means, outlier columns and constant rows included)"""
    assert _rule(M, N) == tile
    ops = _rows_operands(1000 + N + M, M, N, K)
    got = _run_rows(ctx, *ops, act, tile)
    ref, hard, meanb = _consumer_bounds(*ops, act, False, K)
    _check_consumer(f"ln_rows/N{N}/K{K}/{'gelu' if act else 'none'}/M{M}/{tile}", got, ref, hard, meanb, _plain(M))


COLS_CASES = [
    # D (= M = K), N (tokens), tile
    (768, 3304, S128), (768, 3 * 3304, T128), (768, 584, S128), (768, 8, S128),
    (1024, 3304, S128), (1024, 3 * 3304, T128), (1024, 4 * 3304, T256),
]


def _cols_operands(seed, D, N, M=None):
    g = _gen(seed)
    M = M or D
    X16 = _tokens(g, N, D).half()                      # the tokens are the GEMM's columns: the `w` operand
    Wv = _weights(g, M, D)
    mean, _, rstd = _ln_stats(X16.double())
    la, lb = rstd.float(), (mean * rstd).float()
    cs = Wv.double().sum(1).float()
    rb = _noise(g, M) * 0.5
    return Wv, X16, la, lb, cs, rb


def _run_cols(ctx, Wv, X16, la, lb, cs, rb, tile):
    M, K = Wv.shape
    N = X16.shape[0]
    dev = [t.to(DEV) for t in (Wv, X16, la, lb, cs, rb)]
    out = _guarded(M, N, torch.float16, 7.0)
    before = out.clone()
    _launch(ctx, tile, epi=2, M=M, N=N, K=K, out=out, **dict(zip(("in", "w", "ln_a", "ln_b", "ln_cs", "row_bias"), dev)))
    assert _same_bits(out[M:], before[M:]), "guard rows behind the output were written"
    return out[:M].cpu()


@pytest.mark.parametrize("D,N,tile", COLS_CASES)
def test_ln_cols(ctx, D, N, tile):
    """EPI_LN_COLS: V^T = W_v LN(X)^T, out = rstd[n] acc - mur[n] cs[m] + row_bias[m]"""
    assert _rule(D, N) == tile
    ops = _cols_operands(2000 + D + N, D, N)
    got = _run_cols(ctx, *ops, tile)
    ref, hard, meanb = _consumer_bounds(*ops, NONE, True, D)
    _check_consumer(f"ln_cols/D{D}/N{N}/{tile}", got, ref, hard, meanb, (slice(None), _plain(N)))


# -------------------------------------------------------------------------------------------------------------------- split
def _split_planes(x32):
    hi = x32.half()
    return hi, (x32 - hi.float()).half()


def _ulp16(hi):
    """spacing of f16 at hi (2^-24 for zero and subnormals), as float64"""
    _, e = torch.frexp(hi.double().abs())
    e = torch.where(hi == 0, torch.full_like(e, -14), e - 1).clamp(min=-14)
    return torch.ldexp(torch.ones_like(hi, dtype=torch.float64), e - 10)


def _split_operands(seed, M, N, K, teeth, with_scale, res_rows=None):
    """A [M][K], W [N][K], scale, bias, and the residual's planes [res_rows or M][N].  With `teeth` the rows of `_tokens`; without,
    (d): a residual whose low plane is non-zero in every element"""
    g = _gen(seed)
    R = res_rows or M
    A = _noise(g, M, K)
    W16 = _weights(g, N, K)
    scale = (0.05 + 0.1 * torch.rand((N,), generator=g)) if with_scale else None
    bias = torch.round(_noise(g, N) * 32) / 64            # multiples of 2^-6 in [-0.5, 0.5]: exact in f16 next to 1.5
    x0 = _tokens(g, R, N, teeth)
    x0 = torch.where(x0.abs() < 1e-3, torch.full_like(x0, 1e-3), x0)
    hi, lo = _split_planes(x0)
    if teeth and res_rows is None:
        A[5::BIG_MEAN_EVERY] *= 0.05                                    # (a) the product must not drown the mean
        A[7::CONST_EVERY] = 0.0                                         # (c) 0 * w + bias + (1.5 - bias) + 0 = 1.5 in every column
        hi[7::CONST_EVERY] = (1.5 - bias).half()[None, :]
        lo[7::CONST_EVERY] = 0.0
    else:
        fix = (_ulp16(hi) / 4).half()
        lo = torch.where(lo == 0, fix, lo)
        assert bool((lo != 0).all())
    return A.half(), W16, scale, bias, hi, lo


def _split_ref(A16, W16, scale, bias, hi, lo, K, res_index=None):
    A, W = A16.double(), W16.double()
    s = scale.double() if scale is not None else torch.ones(W.shape[0], dtype=torch.float64)
    r = hi.double() + lo.double()
    rmag = hi.double().abs() + lo.double().abs()
    if res_index is not None:
        r, rmag = r[res_index], rmag[res_index]
    x = s[None, :] * (A @ W.T) + bias.double()[None, :] + r
    mag = s.abs()[None, :] * (A.abs() @ W.abs().T) + bias.double().abs()[None, :] + rmag
    return x, mag


def _check_split(tag, K, x, mag, ghi, glo, gstats):
    """ghi / glo [M][N], gstats [chunks][M][2]: the rows the call owns, in GEMM row order"""
    assert bool(torch.isfinite(ghi).all() and torch.isfinite(glo).all() and torch.isfinite(gstats).all()), f"{tag}: unwritten elements"
    got = ghi.double() + glo.double()
    err = (got - x).abs()
    hard = 2.0 ** -21 * x.abs() + (K + 6) * U32 * mag
    meanb = 2.0 ** -21 * x.abs() + math.sqrt(K) * U32 * mag
    r = _record(tag, err, hard, meanb)
    bad = torch.nonzero(err > hard)
    assert bad.numel() == 0, (tag, "first element over the hard bound", bad[0].tolist(), float(err[tuple(bad[0])]), float(hard[tuple(bad[0])]))
    assert err.mean() <= meanb.mean(), (tag, "mean error over the mean bound", r)
    # structure, exact, from the device's output alone
    ulp = _ulp16(ghi)
    assert bool((glo.double().abs() <= ulp / 2).all()), f"{tag}: |lo| > ulp(hi) / 2"
    tie = glo.double().abs() == ulp / 2
    assert bool((((ghi.float() + glo.float()).half() == ghi) | tie).all()), f"{tag}: f16(hi + lo) != hi"
    # statistics per 64-column chunk: sum and centred sum of squares
    M, N = x.shape
    xc = x.view(M, N // 64, 64)
    ec = hard.view(M, N // 64, 64)                      # the error of the device's x, propagated
    s_ref = xc.sum(2)
    s_bound = 64 * U32 * xc.abs().sum(2) + ec.sum(2)
    s_got, q_got = gstats[:, :, 0].double().T, gstats[:, :, 1].double().T
    assert bool(((s_got - s_ref).abs() <= s_bound).all()), (tag, "chunk sums", float(((s_got - s_ref).abs() / s_bound).max()))
    d = xc - (s_ref / 64)[:, :, None]
    q_ref = (d * d).sum(2)
    # first order in the element errors e: 2 sum |d| e; the centre is off by dm <= s_bound / 64, which enters as 64 dm^2; 64 squares
    # and their sum in fp32: (64 + 6) u32 q
    q_bound = 2 * (d.abs() * ec).sum(2) + (ec * ec).sum(2) + 64 * (s_bound / 64) ** 2 + 70 * U32 * q_ref
    assert bool(((q_got - q_ref).abs() <= q_bound).all()), (tag, "centred sums of squares", float(((q_got - q_ref).abs() / q_bound).max()))
    ERRORS[tag]["stats_sum_err_over_bound"] = float(((s_got - s_ref).abs() / s_bound).max())
    ERRORS[tag]["stats_m2_err_over_bound"] = float(((q_got - q_ref).abs() / q_bound.clamp(min=1e-300)).max())
    _dump(tag)


def _run_split(ctx, A16, W16, scale, bias, hi, lo, tile, in_place):
    """-> (hi, lo [M][N], stats [chunks][M][2]) on the host, after checking that nothing else was written"""
    M, K = A16.shape
    N = W16.shape[0]
    dA, dW, dsc, dbi = (None if t is None else t.to(DEV) for t in (A16, W16, scale, bias))
    oh, ol = _guarded(M, N, torch.float16, 7.0), _guarded(M, N, torch.float16, 7.0)
    if in_place:
        oh[:M], ol[:M] = hi.to(DEV), lo.to(DEV)
        rh, rl = oh, ol
    else:
        rh, rl = hi.to(DEV), lo.to(DEV)
    ld = M + GUARD
    stats = torch.full((N // 64, ld, 2), float("nan"), dtype=torch.float32).to(DEV)
    before = [t[M:].clone() for t in (oh, ol)] + [stats[:, M:].clone()]
    _launch(ctx, tile, epi=3, M=M, N=N, K=K, out=oh, out2=ol, res=rh, res2=rl, stats=stats, stats_ld=ld,
            **{"in": dA, "w": dW, "scale": dsc, "bias": dbi})
    assert _same_bits(oh[M:], before[0]) and _same_bits(ol[M:], before[1]), "rows past M of a plane were written"
    assert _same_bits(stats[:, M:], before[2]), "statistics of rows past M were written"
    return oh[:M].cpu(), ol[:M].cpu(), stats[:, :M].cpu()


SPLIT_CASES = [
    # N, K, M, scale, teeth, tile
    (768, 768, 16388, True, True, T256), (768, 768, 8200, False, True, T128), (768, 768, 1276, True, False, S128),       # proj
    (768, 3072, 16388, False, False, T256), (768, 3072, 8200, True, True, T128), (768, 3072, 520, False, True, S128),    # fc2
    (1024, 1024, 12540, True, True, T256), (1024, 1024, 100, False, False, S128),
    (320, 768, 520, True, True, S128), (320, 768, 24580, True, False, T256),                                             # partial n-tile
]


@pytest.mark.parametrize("N,K,M,with_scale,teeth,tile", SPLIT_CASES)
def test_split(ctx, N, K, M, with_scale, teeth, tile):
    """EPI_SPLIT, out of place and in place (as vit_encode runs it): the two planes, their structure, the row statistics, and
    identical bits both ways"""
    assert _rule(M, N) == tile
    ops = _split_operands(3000 + N + K + M, M, N, K, teeth, with_scale)
    x, mag = _split_ref(*ops, K)
    if teeth:    # the teeth hold in the reference itself
        mean, var, _ = _ln_stats(x)
        assert bool((mean[5::BIG_MEAN_EVERY].abs() >= 100 * var[5::BIG_MEAN_EVERY].sqrt()).all())
        assert bool((var[7::CONST_EVERY] == 0).all())
    out = _run_split(ctx, *ops, tile, in_place=False)
    _check_split(f"split/N{N}/K{K}/M{M}/{'scale' if with_scale else 'noscale'}/{tile}", K, x, mag, *out)
    inp = _run_split(ctx, *ops, tile, in_place=True)
    for a, b, what in zip(out, inp, ("hi", "lo", "stats")):
        assert _same_bits(a, b), f"in place and out of place differ in {what}"


PATCH_CASES = [
    # np, npad, B, tile          (3300 patches of the 1035 x 800 page, 576 of a TrOCR crop; row 0 = cls, rows past np + 1 = pad)
    (3300, 3304, 3, T128), (576, 584, 3, S128), (3300, 3304, 5, T256),
]


@pytest.mark.parametrize("np_,npad,B,tile", PATCH_CASES)
def test_split_patch_embedding_mapping(ctx, np_, npad, B, tile):
    """EPI_SPLIT under the periodic row mapping of the patch embedding: GEMM row q -> token row (q / np) npad + 1 + q % np, plus
    row q % np of ONE position table shared by the B images.  cls rows, pad rows, guard rows and their statistics stay untouched."""
    N = K = 768
    M, R = B * np_, B * npad
    assert _rule(M, N) == tile
    A16, W16, scale, bias, ph, pl = _split_operands(4000 + np_ + B, M, N, K, False, False, res_rows=np_)
    q = torch.arange(M)
    x, mag = _split_ref(A16, W16, scale, bias, ph, pl, K, res_index=q % np_)
    rows = (q // np_) * npad + 1 + q % np_
    oh, ol = _guarded(R, N, torch.float16, 7.0), _guarded(R, N, torch.float16, 7.0)
    ld = R + GUARD
    stats = torch.full((N // 64, ld, 2), float("nan"), dtype=torch.float32).to(DEV)
    before = [t.clone() for t in (oh, ol, stats)]
    dev = [t.to(DEV) for t in (A16, W16, bias, ph, pl)]
    _launch(ctx, tile, epi=3, M=M, N=N, K=K, out=oh, out2=ol, stats=stats, stats_ld=ld, row_period=np_, row_stride=npad, row_offset=1,
            **dict(zip(("in", "w", "bias", "res", "res2"), dev)))
    rows_d = rows.to(DEV)
    _check_split(f"split/patch/np{np_}/B{B}/{tile}", K, x, mag, oh[rows_d].cpu(), ol[rows_d].cpu(), stats[:, rows_d].cpu())
    others = torch.ones(R + GUARD, dtype=torch.bool)
    others[rows] = False
    assert int(others.sum()) == B * (npad - np_) + GUARD
    others = others.to(DEV)
    for t, b, what in zip((oh, ol), before, ("hi", "lo")):
        assert _same_bits(t[others], b[others]), f"cls / pad / guard rows of the {what} plane were written"
    assert _same_bits(stats[:, others], before[2][:, others]), "statistics of cls / pad / guard rows were written"


# ------------------------------------------------------------------------------------------- ln_finalize, token_init, the chain
def _finalize(ctx, stats_dev, rows, D, ld):
    rstd = torch.full((rows + GUARD,), float("nan"), dtype=torch.float32).to(DEV)
    mur = rstd.clone()
    before = rstd.clone()
    if DEV == "cuda":
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.ln_finalize(stats_dev.data_ptr(), D // 64, ld, rstd.data_ptr(), mur.data_ptr(), rows, D, EPS)
    ctx.synchronize()
    assert _same_bits(rstd[rows:], before[rows:]) and _same_bits(mur[rows:], before[rows:]), "ln_finalize wrote past `rows`"
    return rstd, mur


def _finalize_bounds(hi, lo):
    """fp64 LayerNorm statistics of x = hi + lo and the first-order bound of what ln_finalize makes of the split epilogue's
    statistics.  The statistics are those of the fp32 x the epilogue held, which hi + lo misses by e <= 2^-11 |lo| + 2^-25 per
    element (the rounding of lo); sums of 64 / of D / 64 terms and the squares are fp32."""
    x = hi.double() + lo.double()
    R, D = x.shape
    mean, var, rstd = _ln_stats(x)
    e = U16 * lo.double().abs() + 2.0 ** -25
    xc, ec = x.view(R, D // 64, 64), e.view(R, D // 64, 64)
    s_bound = 64 * U32 * xc.abs().sum(2) + ec.sum(2)                          # per chunk
    d = xc - (xc.sum(2) / 64)[:, :, None]
    q_bound = 2 * (d.abs() * ec).sum(2) + (ec * ec).sum(2) + 64 * (s_bound / 64) ** 2 + 70 * U32 * (d * d).sum(2)
    dmean = s_bound.sum(1) / D + (D // 64 + 2) * U32 * xc.sum(2).abs().sum(1) / D
    dc = xc.sum(2) / 64 - mean[:, None]                                     # chunk mean - row mean
    ddc = s_bound / 64 + dmean[:, None] + 2 * U32 * ((xc.sum(2) / 64).abs() + mean.abs()[:, None])
    m2 = var * D
    dm2 = q_bound.sum(1) + (64 * (2 * dc.abs() * ddc + ddc * ddc)).sum(1) + (D // 64 + 6) * U32 * m2
    dvar = dm2 / D + 2 * U32 * (var + EPS)
    drstd = 0.5 * rstd ** 3 * dvar + 4 * U32 * rstd                          # d (v + eps)^-1/2 = -1/2 (v + eps)^-3/2 dv; sqrt, 1 / x
    dmur = mean.abs() * drstd + rstd * dmean + 2 * U32 * (mean * rstd).abs()
    return x, mean, rstd, drstd, dmur


@pytest.mark.parametrize("D,K,M", [(768, 768, 1276), (1024, 1024, 780)])
def test_ln_finalize_and_chain(ctx, D, K, M):
    """One block's worth: split producer -> ln_finalize -> rows consumer.  rstd / mean rstd against the fp64 LayerNorm statistics of
    hi + lo; the consumer against fp64 LN(hi + lo) W^T + b — the bound carries the method's own term rstd (|lo| |W|^T): the
    product is taken over the high plane alone ("up to the rounding of x", common.h)."""
    ops = _split_operands(5000 + D, M, D, K, True, True)
    tile = _rule(M, D)
    hi, lo, _ = _run_split(ctx, *ops, tile, in_place=True)
    # the same call again with everything kept on the device, as a block runs
    dA, dW, dsc, dbi = (t.to(DEV) for t in ops[:4])
    oh, ol = _guarded(M, D, torch.float16, 7.0), _guarded(M, D, torch.float16, 7.0)
    oh[:M], ol[:M] = ops[4].to(DEV), ops[5].to(DEV)
    ld = M + GUARD
    stats = torch.full((D // 64, ld, 2), float("nan"), dtype=torch.float32).to(DEV)
    _launch(ctx, tile, epi=3, M=M, N=D, K=K, out=oh, out2=ol, res=oh, res2=ol, stats=stats, stats_ld=ld,
            **{"in": dA, "w": dW, "scale": dsc, "bias": dbi})
    assert _same_bits(oh[:M].cpu(), hi) and _same_bits(ol[:M].cpu(), lo)
    rstd_d, mur_d = _finalize(ctx, stats, M, D, ld)
    x, mean, rstd, drstd, dmur = _finalize_bounds(hi, lo)
    g_rstd, g_mur = rstd_d[:M].cpu().double(), mur_d[:M].cpu().double()
    e_rstd, e_mur = (g_rstd - rstd).abs(), (g_mur - mean * rstd).abs()
    big = torch.arange(5, M, BIG_MEAN_EVERY)
    print(f"ln_finalize D={D}: max err/bound rstd {float((e_rstd / drstd).max()):.3f} mur {float((e_mur / dmur).max()):.3f}; "
          f"rows with |mean| >= 100 std: bound / ref rstd {float((drstd / rstd)[big].max()):.2e} (err {float((e_rstd / rstd)[big].max()):.2e}), "
          f"mur {float((dmur / (mean * rstd).abs())[big].max()):.2e} (err {float((e_mur / (mean * rstd).abs())[big].max()):.2e})")
    ERRORS[f"ln_finalize/D{D}"] = {"rstd_err_over_bound": float((e_rstd / drstd).max()), "mur_err_over_bound": float((e_mur / dmur).max()),
                                   "big_mean_rows_rstd_bound_over_ref": float((drstd / rstd)[big].max()),
                                   "big_mean_rows_rstd_err_over_ref": float((e_rstd / rstd)[big].max())}
    assert bool((e_rstd <= drstd).all()), ("rstd", float((e_rstd / drstd).max()))
    assert bool((e_mur <= dmur).all()), ("mean * rstd", float((e_mur / dmur).max()))
    # consumer over the device's own rstd / mur
    g = _gen(5100 + D)
    N = 2 * D
    W16 = _weights(g, N, D)
    cs = W16.double().sum(1).float()
    bias = _noise(g, N) * 0.5
    out = _guarded(M, N, torch.float16, 7.0)
    keep = [t.to(DEV) for t in (W16, cs, bias)]
    _launch(ctx, _rule(M, N), epi=1, M=M, N=N, K=D, out=out, ln_a=rstd_d, ln_b=mur_d, ln_cs=keep[1], bias=keep[2], **{"in": oh, "w": keep[0]})
    got = out[:M].cpu()
    W = W16.double()
    ref = rstd[:, None] * ((x - mean[:, None]) @ W.T) + bias.double()[None, :]
    absacc = hi.double().abs() @ W.abs().T
    mag = rstd[:, None] * absacc + ((mean * rstd)[:, None] * cs.double()[None, :]).abs() + bias.double().abs()[None, :]
    method = rstd[:, None] * (lo.double().abs() @ W.abs().T)
    stat = drstd[:, None] * absacc + dmur[:, None] * cs.double().abs()[None, :] + (mean * rstd).abs()[:, None] * (U32 * W.abs().sum(1))[None, :]
    base = U16 * ref.abs() + 2.0 ** -25 + method + stat
    _check_consumer(f"chain/D{D}/M{M}", got, ref, base + (D + 4) * U32 * mag, base + math.sqrt(D) * U32 * mag, _plain(M))
    ERRORS[f"chain/D{D}/M{M}"]["method_term_over_u16_ref_mean"] = float(method.mean() / (U16 * ref.abs()).mean())
    _dump(f"chain/D{D}/M{M}")


def test_token_init_split(ctx):
    """cls row and pad rows of every image: hi = f16(cls), lo = f16(cls - hi), zeros in the pad rows, the given statistics in the
    cls row's chunks and zeros in the pad rows'; the token rows between them, and their statistics, stay untouched"""
    B, npad, n_tok, D = 3, 584, 577, 768
    g = _gen(6000)
    cls = _noise(g, D) * 3
    cstats = _noise(g, D // 64, 2)
    R = B * npad
    hi, lo = _guarded(R, D, torch.float16, 7.0), _guarded(R, D, torch.float16, 7.0)
    ld = R + GUARD
    stats = torch.full((D // 64, ld, 2), float("nan"), dtype=torch.float32).to(DEV)
    before = [t.clone() for t in (hi, lo, stats)]
    dcls, dcs = cls.to(DEV), cstats.to(DEV)
    if DEV == "cuda":
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.token_init_split(hi.data_ptr(), lo.data_ptr(), dcls.data_ptr(), dcs.data_ptr(), stats.data_ptr(), ld, B, npad, n_tok, D)
    ctx.synchronize()
    eh, el = _split_planes(cls)
    own = torch.zeros(R + GUARD, dtype=torch.bool)
    for b in range(B):
        r0 = b * npad
        own[r0] = True
        own[r0 + n_tok:r0 + npad] = True
        assert _same_bits(hi[r0].cpu(), eh) and _same_bits(lo[r0].cpu(), el)
        assert bool((hi[r0 + n_tok:r0 + npad] == 0).all() and (lo[r0 + n_tok:r0 + npad] == 0).all())
        assert _same_bits(stats[:, r0].cpu(), cstats)
        assert bool((stats[:, r0 + n_tok:r0 + npad] == 0).all())
    rest = (~own).to(DEV)
    assert _same_bits(hi[rest], before[0][rest]) and _same_bits(lo[rest], before[1][rest]) and _same_bits(stats[:, rest], before[2][:, rest])


# ------------------------------------------------------------------------------- straight-line and bounds-checked copies agree
# M (or N for the column consumer) = a whole number of tiles: every tile runs the straight-line copy.  The same operand rows inside a
# GEMM of 4 more rows (the last tile, 4 rows, runs `body`) and inside one that ends 4 rows into the last full tile (those 4 rows
# run `body` there and the straight-line copy in the first) must come out as the same bits.
PAIR_ROWS = [
    # epi, N, K, act, M_full, tile
    (1, 1536, 768, NONE, 512, S128), (1, 1536, 768, NONE, 4096, T128), (1, 1536, 768, NONE, 8192, T256),
    (1, 3072, 768, GELU, 512, S128), (1, 3072, 768, GELU, 2048, T128), (1, 3072, 768, GELU, 4096, T256),
    (3, 768, 768, NONE, 512, S128), (3, 768, 768, NONE, 8192, T128), (3, 768, 768, NONE, 16384, T256),
]


@pytest.mark.parametrize("epi,N,K,act,Mf,tile", PAIR_ROWS)
def test_straight_line_and_bounds_checked_rows_agree(ctx, epi, N, K, act, Mf, tile):
    bm = TILE_BM[tile]
    Ms = (Mf, Mf + 4, Mf - bm + 4)
    assert all(_rule(M, N) == tile for M in Ms)
    if epi == 1:
        ops = _rows_operands(7000 + N + Mf, Mf + 4, N, K)
        outs = [(_run_rows(ctx, ops[0][:M], ops[1], ops[2][:M], ops[3][:M], ops[4], ops[5], act, tile),) for M in Ms]
    else:
        ops = _split_operands(7000 + N + Mf, Mf + 4, N, K, True, True)
        outs = [_run_split(ctx, ops[0][:M], ops[1], ops[2], ops[3], ops[4][:M], ops[5][:M], tile, in_place=True) for M in Ms]
    for o, M in zip(outs[1:], Ms[1:]):
        n = min(M, Mf)
        for a, b in zip(outs[0], o):
            a, b = (a[:, :n], b[:, :n]) if a.dim() == 3 else (a[:n], b[:n])
            assert _same_bits(a, b), f"rows shared by M = {Mf} and M = {M} differ"


PAIR_COLS = [
    # D, N_full, N_tail (ends 8 columns into the last full n-tile), tile
    (768, 512, 392, S128), (1024, 6400, 6280, T128), (1024, 12288, 12040, T256),
]


@pytest.mark.parametrize("D,Nf,Nt,tile", PAIR_COLS)
def test_straight_line_and_bounds_checked_columns_agree(ctx, D, Nf, Nt, tile):
    Ns = (Nf, Nf + 8, Nt)
    assert all(_rule(D, N) == tile for N in Ns)
    ops = _cols_operands(8000 + D + Nf, D, Nf + 8)
    outs = [_run_cols(ctx, ops[0], ops[1][:N], ops[2][:N], ops[3][:N], ops[4], ops[5], tile) for N in Ns]
    for o, N in zip(outs[1:], Ns[1:]):
        n = min(N, Nf)
        assert _same_bits(outs[0][:, :n], o[:, :n]), f"columns shared by N = {Nf} and N = {N} differ"


PAIR_PLAIN = [
    # N, M_full, tile: the smallest whole-tile N and M_full for which the launcher's rule picks the shape for all three M (the big
    # tiles need 192 of them).  K = 64 is one slice.
    (128, 128, S128), (128, 192 * 256, T128), (256, 192 * 256, T256),
]
_PLAIN_OPS = {}


def _plain_operands(N, Mf):
    """A [Mf + 4][64], W [N][64], bias [N] on the device, made once per case and left unchanged"""
    if (N, Mf) not in _PLAIN_OPS:
        g = _gen(7500 + N + Mf)
        _PLAIN_OPS[(N, Mf)] = tuple(t.to(DEV) for t in (_noise(g, Mf + 4, 64).half(), _weights(g, N, 64), _noise(g, N) * 0.5))
    return _PLAIN_OPS[(N, Mf)]


@pytest.mark.parametrize("act", [NONE, GELU])
@pytest.mark.parametrize("N,Mf,tile", PAIR_PLAIN)
def test_straight_line_and_bounds_checked_plain_f16_agree(ctx, N, Mf, tile, act):
    """the plain epilogue (EPI_NONE), f16 out, no residual, with and without GELU: `f16_fast` against `body`"""
    K, bm = 64, TILE_BM[tile]
    Ms = (Mf, Mf + 4, Mf - bm + 4)
    assert Mf % bm == 0 and N % {T256: 256, T128: 128, S128: 128}[tile] == 0 and all(_rule(M, N) == tile for M in Ms)
    A, W, bias = _plain_operands(N, Mf)
    outs = []
    for M in Ms:
        out = _guarded(M, N, torch.float16, 7.0)
        before = out[M:].clone()
        _launch(ctx, tile, epi=0, M=M, N=N, K=K, act=act, out=out, bias=bias, **{"in": A[:M], "w": W})
        assert _same_bits(out[M:], before), "guard rows behind the output were written"
        assert bool(torch.isfinite(out[:M]).all()), "unwritten or non-finite output elements"
        outs.append(out[:M])
    for o, M in zip(outs[1:], Ms[1:]):
        n = min(M, Mf)
        assert _same_bits(outs[0][:n], o[:n]), f"rows shared by M = {Mf} and M = {M} differ"


def test_every_epilogue_is_cased_on_every_tile_shape():
    """each case asserts the tile shape that ran; this keeps the tables covering all twelve (epilogue, shape) combinations"""
    have = {("rows", c[4]) for c in ROWS_CASES} | {("cols", c[2]) for c in COLS_CASES} | {("split", c[5]) for c in SPLIT_CASES}
    have |= {("plain", c[2]) for c in PAIR_PLAIN}
    assert have == {(e, t) for e in ("rows", "cols", "split", "plain") for t in (T256, T128, S128)}
    assert {c[3] for c in PATCH_CASES} == {T256, T128, S128}


# ----------------------------------------------------------------------------------------------------------- the bench's batch
def test_fc1_at_the_bench_batch(ctx):
    """fc1 (EPI_LN_ROWS + GELU) over R = 64 x 3304 = 211 456 rows: every element finite; fp64 comparison on all rows of the first
    tile, the last tile and 64 tiles drawn with a fixed seed"""
    R, N, K, BM = 64 * 3304, 3072, 768, 256
    assert R % BM == 0 and _rule(R, N) == T256
    g = _gen(9000)
    A16 = torch.empty((R, K), dtype=torch.float16)
    for r0 in range(0, R, 1 << 15):                        # generated in slabs: the fp32 noise of the whole batch is not needed at once
        A16[r0:r0 + (1 << 15)] = _tokens(g, min(1 << 15, R - r0), K).half()
    W16 = _weights(g, N, K)
    cs = W16.double().sum(1).float()
    bias = _noise(g, N) * 0.5
    tiles = sorted({0, R // BM - 1} | set((1 + torch.randperm(R // BM - 2, generator=_gen(9001))[:64]).tolist()))
    rows = torch.cat([torch.arange(t * BM, (t + 1) * BM) for t in tiles])
    assert len(tiles) == 66 and rows.numel() >= 0.05 * R
    la, lb = torch.empty(R, dtype=torch.float32), torch.empty(R, dtype=torch.float32)
    for r0 in range(0, R, 1 << 15):
        mean, _, rstd = _ln_stats(A16[r0:r0 + (1 << 15)].double())
        la[r0:r0 + (1 << 15)], lb[r0:r0 + (1 << 15)] = rstd.float(), (mean * rstd).float()
    dev = [t.to(DEV) for t in (A16, W16, la, lb, cs, bias)]
    out = _guarded(R, N, torch.float16, 7.0)
    guard = out[R:].clone()
    _launch(ctx, T256, epi=1, M=R, N=N, K=K, act=GELU, out=out, **dict(zip(("in", "w", "ln_a", "ln_b", "ln_cs", "bias"), dev)))
    assert bool(torch.isfinite(out[:R]).all()), "unwritten or non-finite output elements"
    assert _same_bits(out[R:], guard), "guard rows behind the output were written"
    got = out[rows.to(DEV)].cpu()
    ref, hard, meanb = _consumer_bounds(A16[rows], W16, la[rows], lb[rows], cs, bias, GELU, False, K)
    _check_consumer(f"ln_rows/fc1/M{R}/sampled{rows.numel()}", got, ref, hard, meanb, _plain(1 << 15).repeat(-(-R // (1 << 15)))[rows])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    """every documented refusal of the launcher comes back as an error, nothing is launched"""
    from marie_icr_amd._lib import PREC_F32, MarieHipError

    M, N, K = 256, 128, 64
    z16 = lambda r, c: torch.zeros((r + GUARD, c), dtype=torch.float16).to(DEV)      # noqa: E731
    zf = lambda n: torch.zeros((n + 8,), dtype=torch.float32).to(DEV)                # noqa: E731
    a, w, out, out2, res, res2 = z16(M, K), z16(N + 8, K), z16(M + 8, N + 8), z16(M + 8, N + 8), z16(M + 8, N + 8), z16(M + 8, N + 8)
    la, lb, cs, bias, rb = zf(M + N), zf(M + N), zf(M + N), zf(M + N), zf(M + N)
    stats = torch.zeros((4, M + GUARD, 2), dtype=torch.float32).to(DEV)
    rows = dict(epi=1, M=M, N=N, K=K, out=out, ln_a=la, ln_b=lb, ln_cs=cs, bias=bias, **{"in": a, "w": w})
    cols = dict(epi=2, M=M, N=N, K=K, out=out, ln_a=la, ln_b=lb, ln_cs=cs, row_bias=rb, **{"in": a, "w": w})
    split = dict(epi=3, M=M, N=N, K=K, out=out, out2=out2, res=res, res2=res2, stats=stats, stats_ld=M + GUARD, bias=bias, **{"in": a, "w": w})
    for base in (rows, cols, split):                       # the bases themselves are accepted
        _launch(ctx, **base)
    bad = [
        ("f32 precision", dict(rows, precision=PREC_F32)),
        ("f32 precision, split", dict(split, precision=PREC_F32)),
        ("N % 8", dict(rows, N=N + 4)),
        ("N % 8, columns", dict(cols, N=N + 4)),
        ("M % 4, rows", dict(rows, M=M + 2)),
        ("M % 4, columns", dict(cols, M=M + 2)),
        ("split, N % 64", dict(split, N=N + 8)),
        ("split without out2", dict(split, out2=None)),
        ("split with GELU", dict(split, act=GELU)),
        ("columns without row_bias", dict(cols, row_bias=None)),
        ("misaligned out", dict(rows, out=out.view(-1)[4:])),
        ("misaligned ln_a", dict(rows, ln_a=la[1:])),
        ("misaligned res2", dict(split, res2=res2.view(-1)[4:])),
    ]
    for what, kw in bad:
        with pytest.raises(MarieHipError):
            _launch(ctx, **kw)
            pytest.fail(f"accepted: {what}")
    if DEV == "cuda":
        torch.cuda.synchronize()
    for t in (out, out2):
        assert bool((t == 0).all()), "a refused call wrote output"
