"""float64 reference of the NHWC convolution primitive (mhip_conv2d_nhwc / mhip_conv2d_nhwc_ex, include/marie_hip.h), written as
plain index arithmetic over the filter taps — a sum of shifted, zero-padded slices — so that it shares no failure mode with a library
convolution (tests/test_conv_ref_cpu.py holds it against torch.nn.functional.conv2d):

  t[b][y][x][n]   = scale[n] * sum_{dy,dx,c} in[b][y*sy + dy*dil - pad][x + dx*dil - pad_x][c] * w[n][dy][dx][c] + bias[n]
  v               = act(t)            without a residual (ReLU or erf GELU)
                  = relu?(t + res)    with one (the residual is added BEFORE the ReLU; GELU with a residual is refused)
  out[b][yp][xp]  = max over the 2x2 / 2x1 window of v, floor: a last odd row / column is dropped

`in` may be two tensors whose channels are concatenated.  With a periodic row mapping, output pixel q (= (b*Ho + y)*Wo + x) takes
residual row q % row_period and lands in buffer row (q / row_period) * row_stride + row_offset + q % row_period (`out_rows`).
Beside the result, `conv_ref` returns the magnitude map |scale| conv(|in|, |w|) + |bias| + |res| the error bounds are made of."""
import math

import torch

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
POOL_NONE, POOL_2x2, POOL_2x1 = 0, 1, 2


def out_size(H, W, KH, KW, sy=1, pad=0, pad_x=-1, dil=1):
    px = pad if pad_x < 0 else pad_x
    return (H + 2 * pad - dil * (KH - 1) - 1) // sy + 1, W + 2 * px - dil * (KW - 1)


def _ceil_div(a, b):
    return -((-a) // b)


def tap_sum(x, w, sy=1, pad=0, pad_x=-1, dil=1):
    """sum over the taps of x [B][H][W][C] (float64) against w [N][KH][KW][C] -> [B][Ho][Wo][N].  Tap (dy, dx) reads input pixel
    (y*sy + dy*dil - pad, x + dx*dil - pad_x); pixels outside the image contribute nothing."""
    B, H, W, C = x.shape
    N, KH, KW, Cw = w.shape
    assert C == Cw and x.dtype == torch.float64 and w.dtype == torch.float64
    px = pad if pad_x < 0 else pad_x
    Ho, Wo = out_size(H, W, KH, KW, sy, pad, px, dil)
    assert Ho > 0 and Wo > 0, "empty output"
    acc = torch.zeros((B, Ho, Wo, N), dtype=torch.float64)
    for dy in range(KH):
        oy = dy * dil - pad                                  # input row of output row y: y*sy + oy
        y0, y1 = max(0, _ceil_div(-oy, sy)), min(Ho - 1, (H - 1 - oy) // sy)
        if y0 > y1:
            continue
        for dx in range(KW):
            ox = dx * dil - px
            x0, x1 = max(0, -ox), min(Wo - 1, W - 1 - ox)
            if x0 > x1:
                continue
            sl = x[:, y0 * sy + oy:y1 * sy + oy + 1:sy, x0 + ox:x1 + ox + 1, :]
            acc[:, y0:y1 + 1, x0:x1 + 1, :] += sl @ w[:, dy, dx, :].T
    return acc


def gelu(t):
    return 0.5 * t * (1.0 + torch.special.erf(t * math.sqrt(0.5)))


def pool_max(v, pool):
    """[B][Ho][Wo][N] -> the max over 2x2 / 2x1 windows with floor (pool 0: v itself)"""
    if pool == POOL_NONE:
        return v
    Hp = v.shape[1] // 2
    rows = torch.maximum(v[:, 0:2 * Hp:2], v[:, 1:2 * Hp:2])
    if pool == POOL_2x1:
        return rows
    Wp = v.shape[2] // 2
    return torch.maximum(rows[:, :, 0:2 * Wp:2], rows[:, :, 1:2 * Wp:2])


def conv_ref(x, w, x2=None, scale=None, bias=None, sy=1, pad=0, pad_x=-1, dil=1, act=ACT_NONE, res=None, pool=POOL_NONE,
             row_period=0):
    """-> dict: `t` (pre-activation, without the residual), `v` (activated, unpooled), `out` (pooled), `mag`, all float64 and
    [B][Ho][Wo][N] but `out` [B][Hp][Wp][N].  x (and x2) [B][H][W][C], w [N][KH][KW][C (+ C2)]; scale, bias [N];
    res [B][Ho][Wo][N] (or [B*Ho*Wo][N]), or [row_period][N] under a periodic row mapping."""
    if res is not None and act == ACT_GELU:
        raise ValueError("GELU is applied before any residual add: refused")
    if res is not None and pool != POOL_NONE:
        raise ValueError("a residual needs an unpooled output")
    if row_period and pool != POOL_NONE:
        raise ValueError("a periodic row mapping needs an unpooled output")
    x, w = x.double(), w.double()
    C1 = x.shape[3]
    acc = tap_sum(x, w[..., :C1].contiguous(), sy, pad, pad_x, dil)
    mag = tap_sum(x.abs(), w[..., :C1].abs().contiguous(), sy, pad, pad_x, dil)
    if x2 is not None:
        x2 = x2.double()
        assert x2.shape[:3] == x.shape[:3] and C1 + x2.shape[3] == w.shape[3]
        acc += tap_sum(x2, w[..., C1:].contiguous(), sy, pad, pad_x, dil)
        mag += tap_sum(x2.abs(), w[..., C1:].abs().contiguous(), sy, pad, pad_x, dil)
    else:
        assert C1 == w.shape[3]
    N = w.shape[0]
    s = torch.ones(N, dtype=torch.float64) if scale is None else scale.double()
    b = torch.zeros(N, dtype=torch.float64) if bias is None else bias.double()
    t = acc * s + b
    mag = mag * s.abs() + b.abs()
    v = t
    if res is not None:
        r = res.double()
        if row_period:
            q = torch.arange(t.shape[0] * t.shape[1] * t.shape[2])
            r = r[q % row_period]
        if r.dim() == 2:                                     # [pixels][N], as the device holds it
            r = r.reshape(t.shape)
        assert r.shape == t.shape
        v = t + r
        mag = mag + r.abs()
    if act == ACT_RELU:
        v = torch.clamp(v, min=0.0)
    elif act == ACT_GELU:
        v = gelu(v)
    return {"t": t, "v": v, "out": pool_max(v, pool), "mag": mag}


def out_rows(M, row_period=0, row_stride=0, row_offset=0):
    """buffer row of every output pixel q in [0, M)"""
    q = torch.arange(M)
    if not row_period:
        return q
    assert row_stride >= row_period
    return (q // row_period) * row_stride + row_offset + q % row_period


def owned(buf_rows, ld, rows, N, pad_cols_writable=False):
    """[buf_rows][ld] bool: the elements a call may write — columns [0, N) of `rows`, and with pad_cols_writable the pad columns
    [N, roundup(N, 8)) of those rows (which come out as zeros)"""
    m = torch.zeros((buf_rows, ld), dtype=torch.bool)
    n_own = min(ld, (N + 7) // 8 * 8) if pad_cols_writable else N
    m[rows, :n_own] = True
    return m
