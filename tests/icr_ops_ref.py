"""TEST INFRASTRUCTURE — float64 statements of the operations behind the non-GEMM kernels of csrc/icr_ops.hip and
csrc/image_ops.hip, the wrong variants ("witnesses") the kernel-level tests must be able to tell from them, and the seeded
inputs both tests/test_icr_ops_ref_cpu.py (no GPU) and tests/test_icr_ops_gpu.py / tests/test_image_ops_gpu.py (MI355X) use.

torch's own op in float64 where one exists (F.conv2d, F.max_pool2d, F.interpolate, F.grid_sample, nn.LSTMCell), numpy in
float64 for the rest (the TPS grid with its constants for any F, H, W; the AttentionCell context; the 16 -> 16 -> 2 score head).
Layouts are the kernels': activations NHWC, filter banks tap-major.  Every input array is what the device gets (fp32 / u8 /
int32, activations already f16-representable); the references read exactly those values and compute in float64.

Inputs whose magnitude depends on a long sum (conv_gray_first, conv_rgb_first, score_head) get their weights rescaled by one
gain, computed from the float64 reference alone, so that the largest output is 1.5: the 1e-3 bar is an absolute one and is
meant for O(1) outputs.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

BAR = 1e-3                 # fp32 mode, and f16 mode where the only f16 step is the output rounding (|out| <= 2: 2^-11 * 2 = 4.9e-4)
PMAX_RTOL = 1e-4           # (C + 4) * 2^-23 = 2.4e-5 at C = 200, a factor of four left
WITNESS = 0.05             # a wrong kernel moves the reference by at least 50 bars


def f16(a):
    """round to the nearest f16, returned as fp32 (what the stage entries narrow exactly)"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _nchw(x):
    return _t(x).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def norm_u8(u8):
    """ToTensor + sub_(0.5).div_(0.5)"""
    return (np.asarray(u8, np.float64) / 255.0 - 0.5) / 0.5


# ------------------------------------------------------------------------------------------------------------ conv_gray_first
def conv_gray_first(img, w9xC, scale, bias, taps_transposed=False, pad_u8_zero=False):
    """img (B, H, W) u8 (normalised here) or float; w9xC (9, C), tap dy*3+dx -> (B, H, W, 64) float64, channels >= C zero.
    Witnesses: the filter read with dy and dx exchanged; the border padded with the u8 value 0, i.e. -1 after normalisation."""
    img = np.asarray(img)
    x = norm_u8(img) if img.dtype == np.uint8 else img.astype(np.float64)
    C = w9xC.shape[1]
    w = np.asarray(w9xC, np.float64).T.reshape(C, 1, 3, 3)
    if taps_transposed:
        w = w.transpose(0, 1, 3, 2)
    xp = F.pad(_t(x)[:, None], (1, 1, 1, 1), value=-1.0 if pad_u8_zero else 0.0)
    y = F.conv2d(xp, _t(w)) * _t(scale).view(1, C, 1, 1) + _t(bias).view(1, C, 1, 1)
    out = np.zeros(x.shape + (64,))
    out[..., :C] = _nhwc(F.relu(y))
    return out


def gray_case(seed, B, H, W, C, u8):
    rng = np.random.default_rng(seed)
    if u8:
        img = rng.integers(0, 256, size=(B, H, W)).astype(np.uint8)
        img[:, 0, 0], img[:, -1, -1] = 0, 255
    else:
        img = rng.uniform(-1, 1, size=(B, H, W)).astype(np.float32)
    w = rng.normal(0, np.sqrt(1 / 3), size=(9, C))
    scale = (1 + rng.uniform(-0.1, 0.1, C)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    pre = conv_gray_first(img, w, scale, np.zeros(C))          # ReLU(s * scale): the gain from the reference alone
    w = (w * (1.4 / pre.max())).astype(np.float32)
    return {"img": img, "w": w, "scale": scale, "bias": bias}


GRAY_SHAPES = [(1, 3, 5), (2, 7, 13), (3, 32, 100)]       # 15 pixels (under one block), 182 (a partial last block), production
GRAY_CASES = [(f"{'u8' if u8 else 'f32in'}-C{C}-{B}x{H}x{W}", dict(seed=100 + 10 * i + C + u8, B=B, H=H, W=W, C=C, u8=u8))
              for u8 in (True, False) for C in (20, 32, 64) for i, (B, H, W) in enumerate(GRAY_SHAPES)]


# ------------------------------------------------------------------------------------------------------------ max / avg pools
def maxpool_s21_p01(x, pad_zero=False):
    """nn.MaxPool2d(2, (2, 1), (0, 1)) on NHWC.  Witness: the padding columns count as 0 instead of never winning."""
    t = _nchw(x)
    if pad_zero:
        return _nhwc(F.max_pool2d(F.pad(t, (1, 1, 0, 0), value=0.0), 2, (2, 1)))
    return _nhwc(F.max_pool2d(t, 2, (2, 1), (0, 1)))


def maxpool(x, k, pad_zero=False):
    """k = 2: nn.MaxPool2d(2, 2);  k = 3: nn.MaxPool2d(3, 1, 1).  Witness (k = 3): padding counts as 0."""
    t = _nchw(x)
    if k == 2:
        return _nhwc(F.max_pool2d(t, 2, 2))
    if pad_zero:
        return _nhwc(F.max_pool2d(F.pad(t, (1, 1, 1, 1), value=0.0), 3, 1))
    return _nhwc(F.max_pool2d(t, 3, 1, 1))


def pool_input(seed, shape, negative):
    """f16-representable N(0, 1) entries; `negative`: every entry below -0.1"""
    x = np.random.default_rng(seed).normal(0, 1, size=shape)
    return f16(-np.abs(x) - 0.1 if negative else x)


# (B, H, W, C), negative, precisions
S21_CASES = [("1x2x1x8", (1, 2, 1, 8), False, ("f16", "f32")),         # every output sees a single column
             ("1x5x4x16-neg", (1, 5, 4, 16), True, ("f16", "f32")),    # odd H: the last row is dropped
             ("2x8x25x256", (2, 8, 25, 256), False, ("f16", "f32")),
             ("1x5x4x4-neg", (1, 5, 4, 4), True, ("f32",))]
MAXPOOL_CASES = [("k2-1x2x2x8", 2, (1, 2, 2, 8), False, ("f16", "f32")),
                 ("k2-1x5x7x16-neg", 2, (1, 5, 7, 16), True, ("f16", "f32")),     # odd sizes floor
                 ("k2-3x32x100x64", 2, (3, 32, 100, 64), False, ("f16", "f32")),
                 ("k3-1x1x1x8", 3, (1, 1, 1, 8), False, ("f16", "f32")),
                 ("k3-1x3x4x16-neg", 3, (1, 3, 4, 16), True, ("f16", "f32")),
                 ("k3-1x6x5x512", 3, (1, 6, 5, 512), False, ("f16", "f32")),
                 ("k3-1x1500x1400x8", 3, (1, 1500, 1400, 8), False, ("f16",))]    # 2.1 M outputs: a second grid-stride trip


def avgpool_hw(x):
    """nn.AdaptiveAvgPool2d(1) on (B, HW, C)"""
    return np.asarray(x, np.float64).mean(axis=1)


AVG_SHAPES = [(1, 1, 1), (2, 7, 20), (3, 48, 512)]


def avg_input(seed, shape):
    return f16(0.8 + 0.1 * np.random.default_rng(seed).normal(size=shape))


# ------------------------------------------------------------------------------------------------------------ TPS
def tps_fiducials(Fn):
    """C of GridGenerator: Fn / 2 points along the top edge, Fn / 2 along the bottom edge of [-1, 1]^2"""
    half = Fn // 2
    xs = np.linspace(-1.0, 1.0, half)
    return np.concatenate([np.stack([xs, -np.ones(half)], 1), np.stack([xs, np.ones(half)], 1)], 0)


def _rbf(d2, eps=0.0):
    """r^2 log(r + eps) from squared distances"""
    r = np.sqrt(d2)
    return d2 * np.log(np.where(d2 > 0, r, 1.0) + eps)


def tps_constants(Fn, H, W):
    """inv_delta_C (Fn+3, Fn+3) and P_hat (H*W, Fn+3) in float64 from their formulas:
         delta_C = [[1, C, R], [0, C^T], [0, 1^T]] with R_ij = r_ij^2 log r_ij (0 on the diagonal),
         P_hat   = [1, P, |P - C_j|^2 log(|P - C_j| + 1e-6)], P the pixel centres (2 i + 1 - n) / n, x fastest."""
    C = tps_fiducials(Fn)
    R = _rbf(((C[:, None] - C[None]) ** 2).sum(-1))
    delta = np.zeros((Fn + 3, Fn + 3))
    delta[:Fn, 0], delta[:Fn, 1:3], delta[:Fn, 3:] = 1.0, C, R
    delta[Fn:Fn + 2, 3:] = C.T
    delta[Fn + 2, 3:] = 1.0
    gx = (2 * np.arange(W) + 1.0 - W) / W
    gy = (2 * np.arange(H) + 1.0 - H) / H
    P = np.stack(np.meshgrid(gx, gy), axis=2).reshape(-1, 2)
    P_hat = np.concatenate([np.ones((H * W, 1)), P, _rbf(((P[:, None] - C[None]) ** 2).sum(-1), 1e-6)], 1)
    return np.linalg.inv(delta), P_hat


def tps_grid(c_prime, inv_delta_c, p_hat):
    """GridGenerator.build_P_prime: (B, Fn, 2) -> (B, H*W, 2), float64"""
    c_prime = np.asarray(c_prime, np.float64)
    cz = np.concatenate([c_prime, np.zeros((c_prime.shape[0], 3, 2))], 1)
    return np.asarray(p_hat, np.float64)[None] @ (np.asarray(inv_delta_c, np.float64)[None] @ cz)


def tps_sample(crops, c_prime, inv_delta_c, p_hat, align_corners=True, padding_mode="border", ignore_b=False):
    """the rectified, normalised crops (B, H, W).  Witnesses: align_corners=False; zero padding; every image sampled from
    crop 0."""
    B, H, W = crops.shape
    grid = _t(tps_grid(c_prime, inv_delta_c, p_hat).reshape(B, H, W, 2))
    x = _t(norm_u8(crops[:1].repeat(B, 0) if ignore_b else crops))[:, None]
    return F.grid_sample(x, grid, mode="bilinear", padding_mode=padding_mode, align_corners=align_corners)[:, 0].numpy()


def tps_identity_expected(crops):
    """What the identity fiducials give, in closed form: P holds pixel CENTRES, (2 i + 1 - n) / n, and grid_sample reads them with
    align_corners=True, so output pixel i samples the crop at (i + 0.5) (n - 1) / n — the crop shrunk by (n - 1) / n about its
    centre, not the crop itself.  Plain bilinear interpolation in float64, no TPS constants involved."""
    n = norm_u8(crops)
    B, H, W = n.shape
    fy, fx = (np.arange(H) + 0.5) * (H - 1) / H, (np.arange(W) + 0.5) * (W - 1) / W
    y0, x0 = np.floor(fy).astype(int), np.floor(fx).astype(int)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    wy, wx = (fy - y0)[None, :, None], (fx - x0)[None, None, :]
    top = n[:, y0][:, :, x0] * (1 - wx) + n[:, y0][:, :, x1] * wx
    bot = n[:, y1][:, :, x0] * (1 - wx) + n[:, y1][:, :, x1] * wx
    return top * (1 - wy) + bot * wy


def tps_clamped(c_prime, inv_delta_c, p_hat):
    """per sample: which side of [-1, 1]^2 the grid leaves -> bool (B, H*W, 4) = left, right, top, bottom"""
    g = tps_grid(c_prime, inv_delta_c, p_hat)
    return np.stack([g[..., 0] < -1, g[..., 0] > 1, g[..., 1] < -1, g[..., 1] > 1], -1)


def tps_crops(B, H, W):
    """Smooth crops: a diagonal sinusoid sin(k (x' + y') + phase) quantised to u8, run from a different corner per image.
    Neighbouring pixels differ by at most k + 1/255 <= 0.1 in normalised units.  Where the crop is large enough for an odd
    number of half periods along the diagonal at k <= 0.092, the start corner is exactly 0 and the opposite one 255."""
    steps = H + W - 2
    m = int(0.092 * steps / np.pi)
    m -= 1 - m % 2                                   # the largest odd count of half periods, or <= 0
    k, phase = (m * np.pi / steps, -np.pi / 2) if m >= 1 else (0.092, 0.3)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((B, H, W), np.uint8)
    for b in range(B):
        xx = W - 1 - x if b % 3 == 1 else x
        yy = H - 1 - y if b % 3 == 2 else y
        out[b] = np.rint((np.sin(k * (xx + yy) + phase) * 0.5 + 0.5) * 255.0)
    return out


def tps_case(Fn, H, W, B, kind, seed=7):
    inv, p_hat = tps_constants(Fn, H, W)
    C = tps_fiducials(Fn)
    if kind == "identity":
        cp = np.repeat(C[None], B, 0)
    elif kind == "jitter":
        cp = C[None] + np.random.default_rng(seed + B).uniform(-0.15, 0.15, size=(B, Fn, 2))
    else:
        cp = np.repeat(C[None] * 1.5, B, 0)
    return {"crops": tps_crops(B, H, W), "c_prime": cp.astype(np.float32), "inv_delta_c": inv.astype(np.float32),
            "p_hat": p_hat.astype(np.float32)}


TPS_CASES = [(f"F{Fn}-{H}x{W}-B{B}-{kind}", dict(Fn=Fn, H=H, W=W, B=B, kind=kind))
             for (Fn, H, W) in ((6, 4, 6), (20, 32, 100)) for B in (1, 3) for kind in ("identity", "jitter", "x1.5")]


# ------------------------------------------------------------------------------------------------------------ attention cell
def attn_scores(hproj, hp256, score_w):
    """e (B, T) = score(tanh(i2h(H) + h2h(h)))"""
    return np.tanh(np.asarray(hproj, np.float64) + np.asarray(hp256, np.float64)[:, None]) @ np.asarray(score_w, np.float64)


def attn_alpha(e):
    e = e - e.max(axis=1, keepdims=True)
    p = np.exp(e)
    return p / p.sum(axis=1, keepdims=True)


def attn_context(hproj, hp256, score_w, H, softmax_over_64=False):
    """context (B, 256) = softmax_T(e)^T H.  Witness: the soft-max taken over 64 score slots whatever T is (the slots behind
    T holding 0)."""
    e = attn_scores(hproj, hp256, score_w)
    T = e.shape[1]
    if softmax_over_64:
        e = np.concatenate([e, np.zeros((e.shape[0], 64 - T))], 1)
    return np.einsum("bt,btj->bj", attn_alpha(e)[:, :T], np.asarray(H, np.float64))


def attn_context_case(T, B, ld_hp, sharp, seed=11):
    rng = np.random.default_rng(seed + 7 * T + B)
    hp = np.full((B, ld_hp), np.nan, np.float32)                      # columns >= 256 must not be read
    hp[:, :256] = rng.normal(0, 0.5, size=(B, 256))
    H = f16(rng.uniform(-1, 1, size=(1, 1, 256)) + 0.3 * rng.normal(size=(B, T, 256)))    # O(1) with a per-channel offset
    return {"hproj": rng.normal(0, 1, size=(B, T, 256)).astype(np.float32), "hp": hp,
            "score_w": (rng.normal(0, 0.09, size=256) * (8 if sharp else 1)).astype(np.float32), "H": H}


ATTN_CONTEXT_CASES = [(f"T{T}-B{B}-ld{ld}-{'sharp' if sharp else 'flat'}", dict(T=T, B=B, ld_hp=ld, sharp=sharp))
                      for T in (1, 26, 64) for B, ld in ((1, 256), (3, 1280)) for sharp in (False, True)]


def lstm_cell(gates, c_prev):
    """nn.LSTMCell's state update in float64 on given gate pre-activations (B, 1024), rows i, f, g, o: an LSTMCell whose
    W_ih is the identity and whose W_hh and biases are zero -> (h, c)"""
    cell = torch.nn.LSTMCell(1024, 256, bias=False, dtype=torch.float64)
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(1024, dtype=torch.float64))
        cell.weight_hh.zero_()
        h, c = cell(_t(gates), (torch.zeros(gates.shape[0], 256, dtype=torch.float64), _t(c_prev)))
    return h.numpy(), c.numpy()


def attn_cell(gctx, ghid1024, w_onehot, chars, c_prev, gate_order="ifgo", chars_from_row0=False):
    """gates = gctx + ghid + w_onehot[chars] -> (h, c).  Witnesses: the gate blocks read in the order i, g, f, o; the one-hot
    row of chars[0] used for every batch row."""
    chars = np.asarray(chars)
    rows = np.asarray(w_onehot, np.float64)[np.full_like(chars, chars[0]) if chars_from_row0 else chars]
    gates = (np.asarray(gctx, np.float64) + np.asarray(ghid1024, np.float64) + rows).reshape(-1, 4, 256)
    gates = gates[:, ["ifgo".index(g) for g in gate_order]].reshape(-1, 1024)
    return lstm_cell(gates, np.asarray(c_prev, np.float64))


NUM_CLASS = 96


def attn_cell_case(B, seed=23):
    """the three addends N(0, 2/3) each (the pre-activations N(0, 2)), a few of them at +-100; ghid columns 0..255 NaN"""
    rng = np.random.default_rng(seed + B)
    s = np.sqrt(2 / 3)
    gctx = rng.normal(0, s, size=(B, 1024)).astype(np.float32)
    pos = rng.choice(1024, size=12, replace=False)
    gctx[:, pos] = np.where(np.arange(12) % 2 == 0, 100.0, -100.0).astype(np.float32)     # 3 in each gate block on average
    ghid = np.full((B, 1280), np.nan, np.float32)
    ghid[:, 256:] = rng.normal(0, s, size=(B, 1024))
    chars = np.array([0, 95, 41][:B] if B > 1 else [95], np.int32)
    return {"gctx": gctx, "ghid": ghid, "w_onehot": rng.normal(0, s, size=(NUM_CLASS, 1024)).astype(np.float32), "chars": chars,
            "c_prev": rng.uniform(-1, 1, size=(B, 256)).astype(np.float32)}


# ------------------------------------------------------------------------------------------------------------ arg-max
def argmax_rows(logits, C):
    """torch.max(x[:, :C], 1).indices: the first maximum; the first NaN if there is one; 0 for a row of -inf"""
    return torch.max(torch.from_numpy(np.ascontiguousarray(logits[:, :C])), 1).indices.numpy().astype(np.int32)


def softmax_pmax(logits):
    """float64 soft-max probability of the maximum"""
    x = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore"):
        return 1.0 / np.exp(x - x.max(axis=1, keepdims=True)).sum(axis=1)


ARGMAX_C = (1, 64, 65, 96, 200)


def argmax_rows_case(C, seed=31):
    """rows (n, C) fp32 and what each is: plain rows, one spanning -80 .. +40, ties across lanes and within a lane (columns c
    and c + 64), then the non-finite rows (from index `first_nonfinite` on)"""
    rng = np.random.default_rng(seed + C)
    rows, names = [], []
    for _ in range(3):
        rows.append(rng.normal(0, 2, C)), names.append("plain")
    rows.append(rng.uniform(-80, 40, C)), names.append("span")
    if C >= 2:
        r = rng.normal(0, 1, C)
        a, b = sorted(rng.choice(min(C, 64), 2, replace=False))       # two different lanes
        r[[a, b]] = 7.0
        rows.append(r), names.append("tie-lanes")
    if C > 64:
        r = rng.normal(0, 1, C)
        c = int(rng.integers(0, C - 64))
        r[[c, c + 64]] = 7.0                                          # the same lane, two trips
        rows.append(r), names.append("tie-lane")
        r = rng.normal(0, 1, C)
        r[[c + 64, (c + 5) % 64]] = 7.0                               # the later trip of one lane against another lane
        rows.append(r), names.append("tie-mixed")
    first_nonfinite = len(rows)
    rows.append(np.full(C, -np.inf)), names.append("all-minus-inf")
    r = rng.normal(0, 1, C)
    r[-1] = np.nan
    rows.append(r), names.append("nan-last")
    if C > 70:
        r = rng.normal(0, 1, C)
        r[[3, 70]] = np.nan
        r[1] = 9.0
        rows.append(r), names.append("nan-3-70")
    return np.stack(rows).astype(np.float32), names, first_nonfinite


# ------------------------------------------------------------------------------------------------------------ conv_rgb_first
def conv_rgb_first(img, H, W, w27x64, scale, bias, channels_reversed=False, canvas_pad_zero=False, f16_emulated=False):
    """img (th, tw, 3) u8 top-left on an (H, W) canvas of u8 zeros -> (v - 127.5) / 127.5 -> conv3x3 pad 1 (w27x64[k][n], k =
    (dy*3+dx)*3 + c) -> scale / bias -> ReLU -> (H, W, 64) float64.  Witnesses: the colour channels read in reverse; the canvas
    padding taken as 0 AFTER the normalisation.  f16_emulated: pixels and filters rounded to f16, float64 in between, the
    output rounded to f16 (the MFMA kernel's rounding points)."""
    th, tw = img.shape[:2]
    x = np.full((H, W, 3), 0.0 if canvas_pad_zero else -1.0)
    x[:th, :tw] = (img.astype(np.float64) - 127.5) / 127.5
    if channels_reversed:
        x = x[..., ::-1]
    w = np.asarray(w27x64, np.float64)
    if f16_emulated:
        x, w = f16(x).astype(np.float64), f16(w).astype(np.float64)
    wt = w.reshape(3, 3, 3, 64).transpose(3, 2, 0, 1)                   # [n][c][dy][dx]
    y = F.conv2d(_nchw(x[None]), _t(wt), padding=1) * _t(scale).view(1, 64, 1, 1) + _t(bias).view(1, 64, 1, 1)
    out = _nhwc(F.relu(y))[0]
    return f16(out).astype(np.float64) if f16_emulated else out


RGB_SHAPES = [(3, 5, 3, 5), (17, 23, 17, 23), (30, 45, 32, 64), (520, 512, 520, 512)]     # th, tw, H, W


def rgb_case(th, tw, H, W, seed=41):
    rng = np.random.default_rng(seed + th)
    img = (rng.integers(0, 256, size=(th, tw, 3)) * np.array([1.0, 0.6, 0.3])).astype(np.uint8)    # channels scaled differently
    w = rng.normal(0, 1, size=(27, 64))
    scale = (1 + rng.uniform(-0.1, 0.1, 64)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, 64).astype(np.float32)
    w = (w * (1.4 / conv_rgb_first(img, H, W, w, scale, np.zeros(64)).max())).astype(np.float32)
    return {"img": img, "H": H, "W": W, "w": w, "scale": scale, "bias": bias}


# ------------------------------------------------------------------------------------------------------------ upsample
def upsample_bilinear(x, Ho, Wo, align_corners=False):
    """F.interpolate(size=(Ho, Wo), mode='bilinear', align_corners=False) on NHWC.  Witness: align_corners=True."""
    return _nhwc(F.interpolate(_nchw(x), size=(Ho, Wo), mode="bilinear", align_corners=align_corners))


# (B, Hi, Wi, C), (Ho, Wo), precisions
UPSAMPLE_CASES = [("1x1x1x8-2x2", (1, 1, 1, 8), (2, 2), ("f16", "f32")),
                  ("1x3x4x64-6x8", (1, 3, 4, 64), (6, 8), ("f16", "f32")),
                  ("2x5x3x16-7x8", (2, 5, 3, 16), (7, 8), ("f16", "f32")),
                  ("1x725x725x8-1450x1450", (1, 725, 725, 8), (1450, 1450), ("f16",))]    # 2.1 M outputs: past the grid cap


def upsample_input(seed, shape):
    return f16(np.random.default_rng(seed).uniform(-1.5, 1.5, size=shape))


# ------------------------------------------------------------------------------------------------------------ score head
def score_head(x16, w1, b1, w2, b2, w2_rows_swapped=False, no_relu=False, f16_emulated=False):
    """ReLU(x W1^T + b1) W2^T + b2 per pixel: x16 (npix, 16) -> (npix, 2) float64.  Witnesses: the two rows of w2 exchanged;
    the hidden ReLU missing.  f16_emulated: the hidden activation rounded to f16 after the ReLU (the f16 kernel's one
    rounding point; its input is f16 already and its scores are fp32)."""
    h = np.asarray(x16, np.float64) @ np.asarray(w1, np.float64).T + np.asarray(b1, np.float64)
    if not no_relu:
        h = np.maximum(h, 0.0)
    if f16_emulated:
        h = f16(h).astype(np.float64)
    w2 = np.asarray(w2, np.float64)
    return h @ (w2[::-1] if w2_rows_swapped else w2).T + np.asarray(b2, np.float64)


SCORE_CASES = [("stride16-n1", 16, 1, ("f16", "f32")), ("stride64-n1", 64, 1, ("f16", "f32")),
               ("stride16-n257", 16, 257, ("f16", "f32")), ("stride64-n257", 64, 257, ("f16", "f32")),
               ("stride16-n2100000", 16, 2_100_000, ("f16",))]                        # past the 8192-block cap


def score_case(stride, npix, seed=53):
    rng = np.random.default_rng(seed + stride + npix % 1000)
    x = np.full((npix, stride), np.nan, np.float32)                # channels 16.. must not be read
    x[:, :16] = f16(rng.uniform(0, 1, size=(npix, 16)))
    w1 = rng.uniform(-0.5, 0.5, size=(16, 16)).astype(np.float32)
    b1 = rng.uniform(-0.1, 0.1, 16).astype(np.float32)
    w2, b2 = rng.uniform(-0.5, 0.5, size=(2, 16)), rng.uniform(-0.1, 0.1, 2)
    if npix == 1:
        w2[0], w2[1] = np.abs(w2[0]), -np.abs(w2[1])               # one pixel: keep the two scores apart for the row witness
    g = 1.5 / np.abs(score_head(x[:, :16], w1, b1, w2, b2)).max()
    return {"x": x, "w1": w1, "b1": b1, "w2": (w2 * g).astype(np.float32), "b2": (b2 * g).astype(np.float32)}


# ------------------------------------------------------------------------------------------------------------ resize
RESIZE_CASES = [((1, 1), (3, 3)), ((7, 9), (7, 9)), ((40, 30), (64, 48)), ((330, 255), (165, 128)), ((50, 300), (20, 301))]


def resize_linear_u8(img, dh, dw):
    from oracle.craft_ref import cv_resize_linear_u8

    return cv_resize_linear_u8(img, dw, dh)
