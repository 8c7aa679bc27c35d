"""ORACLE-SIDE TEST INFRASTRUCTURE (not product code) — the bidirectional LSTM recurrence in fp64, the error bound of the HIP
kernels against it, an fp32 / f16 emulation of the kernels' arithmetic with named bugs, and the seeded operand sets the
kernel-level tests feed to ``mhip_lstm_rec_host`` (csrc/lstm.hip).

Layouts, all in PyTorch's order (``nn.LSTM(input, 256, bidirectional=True, batch_first=True)``, h0 = c0 = 0):
    whh    [2][1024][256]    weight_hh_l0, weight_hh_l0_reverse; gate rows i, f, g, o
    xproj  [B][T][2][1024]   x_t W_ih^T + b_ih + b_hh per direction, gate-major
    h      [B][T][512]       forward | reverse; the reverse direction walks t = T-1 .. 0

``reference_forced`` is teacher-forced: step t of a direction consumes the DEVICE's h of that direction's previous step, so the
matrix product sees exactly the operand the kernel fed to its own (what it wrote out, f16-rounded in the f16 mode) and every
step is compared at rounding level — a free-running comparison would grow chaotically over 63 steps.  The cell state is not
visible from outside and is carried by the reference itself in fp64; the bound carries the device's drift from it (E_c).

The bound, to first order (the cross terms of second order that cost nothing are kept) from u16 = 2^-11, u32 = 2^-24 and
magnitudes the reference computes.  p is a pre-activation, L = log2 e, dL = |fl32(L) - L| / L = 1.3e-8:
    pre-activation  dpre = (256 + 1) u32 (|xproj| + |h_prev| |W|^T): fp32 accumulation of 256 terms in any order and the add of
                    xproj; the f16 x f16 products are exact in fp32, the fp32 products round once inside the fused multiply-add
    sigmoid         rcp(1 + exp2(-fl(L) p)):  e = exp2(..) carries the relative error dpre + |p| (u32 + dL) (the constant and the
                    rounding of the product) + 2 u32 (v_exp_f32: 1 ulp <= 2^-23 relative); d sigma / d ln e = -sigma (1 - sigma).
                    The add rounds (u32) and v_rcp_f32 is 1 ulp (2 u32), both relative to sigma:
                        ds = sigma (1 - sigma) (dpre + |p| (u32 + dL) + 2 u32) + 3 u32 sigma
    tanh            1 - 2 r, r = rcp(1 + exp2(2 fl(L) p)):  ln e = 2 p, so e carries 2 dpre + 2 |p| (u32 + dL) + 2 u32, and
                    d tanh / d ln e = (1 - tanh^2) / 2;  r carries 3 u32 r as above, 2 r = 1 - tanh, the subtraction rounds:
                        dt = (1 - tanh^2) (dpre + |p| (u32 + dL) + u32) + 3 u32 (1 - tanh) + u32 |tanh|
    cell            c = f c_prev + i g with three roundings:
                        E_c = (f + df) E_c_prev + |c_prev| df + |g| di + (i + di) dg + 2 u32 (|f c_prev| + |i g|)
                    which contracts because f < 1 and so stays finite over any number of steps
    output          h = o tanh(c), tanh(c) with E_c in the place of dpre, the product rounds, the store rounds to the output type:
                        |h_dev - h| <= u_out |h| + sub + (1 + u_out) (|tanh c| do + (o + do) dt(c) + u32 |h|)
                    u_out = u16, sub = 2^-25 (half the spacing of f16 subnormals) in the f16 mode; u_out = u32, sub = 0 in fp32
The mean form replaces 256 + 1 by sqrt(256): the probabilistic accumulation bound, as tests/test_gemm_fold_gpu.py has it.

Only ``tests/`` may import this module.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

HID = 256
U16, U32 = 2.0 ** -11, 2.0 ** -24
L2E = 1.4426950408889634                                 # the constant of fast_sigmoid / fast_tanh (csrc/lstm.hip)
DL = abs(float(np.float32(L2E)) - math.log2(math.e)) / math.log2(math.e)
ARG = U32 + DL                                           # relative error of fl(fl(L) p)
K_HARD, K_MEAN = HID + 1.0, math.sqrt(HID)
F32 = np.float32

# the c mutation scales the cell state once by 1 - C_EPS.  At 1e-3 it moves the f16 emulation by only 6 .. 16 x the bound (the
# bound there is the f16 rounding of h, u16 |h| = 4.9e-4 |h|, against d h = o (1 - tanh^2 c) c eps); the effect is linear in eps,
# and 1e-2 gives 61 .. 155 x (fp32: 197 .. 403 x), clear of the 10 x the CPU test asks of every mutation.
C_EPS = 1e-2

MUTATIONS = ("zero_fragment", "swap_units", "stale_h", "reverse_walks_forward", "swap_f_i", "scale_c")


def rounded(a: np.ndarray, f16: bool) -> np.ndarray:
    """the operand as the kernel sees it (fp32 array holding f16-representable values in the f16 mode)"""
    return a.astype(np.float16).astype(np.float32) if f16 else a.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ fp64
def _sigmoid(p):
    """(sigma(p), 1 - sigma(p)), each without cancellation"""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-p)), 1.0 / (1.0 + np.exp(p))


def _tanh(p):
    """(tanh(p), 1 - tanh(p)^2), the second without cancellation"""
    e = np.exp(-2.0 * np.abs(p))
    return np.tanh(p), 4.0 * e / (1.0 + e) ** 2


def _gates(pre):
    return pre[..., :HID], pre[..., HID:2 * HID], pre[..., 2 * HID:3 * HID], pre[..., 3 * HID:]


def _time(d: int, s: int, T: int) -> int:
    return s if d == 0 else T - 1 - s


def reference_free(whh: np.ndarray, xproj: np.ndarray) -> np.ndarray:
    """the plain bidirectional LSTM in fp64 -> h [B][T][512]"""
    B, T = xproj.shape[:2]
    W, x = whh.astype(np.float64), xproj.astype(np.float64)
    out = np.zeros((B, T, 2 * HID))
    for d in range(2):
        h, c = np.zeros((B, HID)), np.zeros((B, HID))
        for s in range(T):
            t = _time(d, s, T)
            pi, pf, pg, po = _gates(x[:, t, d] + h @ W[d].T)
            c = _sigmoid(pf)[0] * c + _sigmoid(pi)[0] * np.tanh(pg)
            h = _sigmoid(po)[0] * np.tanh(c)
            out[:, t, d * HID:(d + 1) * HID] = h
    return out


def _d_sigmoid(p, s, s1, dpre):
    return s * s1 * (dpre + np.abs(p) * ARG + 2 * U32) + 3 * U32 * s


def _d_tanh(p, t, t1, dpre):
    return t1 * (dpre + np.abs(p) * ARG + U32) + 3 * U32 * (1.0 - t) + U32 * np.abs(t)


def reference_forced(whh_rounded: np.ndarray, xproj: np.ndarray, h_dev: np.ndarray, f16: bool) -> Dict[str, np.ndarray]:
    """h_dev [B][T][512]: what the device wrote.  -> {"h": reference h, "bound": per-element worst-case bound, "mean_bound": the
    per-element probabilistic form, "c_max": max |c| the reference reached} (module docstring)"""
    B, T = xproj.shape[:2]
    W, x, hd = whh_rounded.astype(np.float64), xproj.astype(np.float64), h_dev.astype(np.float64)
    Wabs = np.abs(W)
    u_out, sub = (U16, 2.0 ** -25) if f16 else (U32, 0.0)
    kk = np.array([K_HARD, K_MEAN]).reshape(2, 1, 1)                  # both forms side by side on a leading axis
    h_ref = np.zeros((B, T, 2 * HID))
    bound = np.zeros((2, B, T, 2 * HID))
    c_max = 0.0
    for d in range(2):
        cols = slice(d * HID, (d + 1) * HID)
        c, Ec = np.zeros((B, HID)), np.zeros((2, B, HID))
        for s in range(T):
            t = _time(d, s, T)
            hp = hd[:, _time(d, s - 1, T), cols] if s else np.zeros((B, HID))
            pre = x[:, t, d] + hp @ W[d].T
            dpre = kk * U32 * (np.abs(x[:, t, d]) + np.abs(hp) @ Wabs[d].T)
            pi, pf, pg, po = _gates(pre)
            qi, qf, qg, qo = _gates(dpre)
            (i, i1), (f, f1), (o, o1) = _sigmoid(pi), _sigmoid(pf), _sigmoid(po)
            g, g1 = _tanh(pg)
            di, df, do = _d_sigmoid(pi, i, i1, qi), _d_sigmoid(pf, f, f1, qf), _d_sigmoid(po, o, o1, qo)
            dg = _d_tanh(pg, g, g1, qg)
            Ec = (f + df) * Ec + np.abs(c) * df + np.abs(g) * di + (i + di) * dg + 2 * U32 * (np.abs(f * c) + np.abs(i * g))
            c = f * c + i * g
            tc, tc1 = _tanh(c)
            h = o * tc
            core = np.abs(tc) * do + (o + do) * _d_tanh(c, tc, tc1, Ec) + U32 * np.abs(h)
            h_ref[:, t, cols] = h
            bound[:, :, t, cols] = u_out * np.abs(h) + sub + (1.0 + u_out) * core
            c_max = max(c_max, float(np.abs(c).max()))
    return {"h": h_ref, "bound": bound[0], "mean_bound": bound[1], "c_max": c_max}


# ------------------------------------------------------------------------------------- the kernels' arithmetic, in numpy
def _fast_sigmoid(x):
    """fast_sigmoid of csrc/lstm.hip in fp32 (libm's exp2 in the place of v_exp_f32): exp2 -> inf -> 1 / inf = 0"""
    with np.errstate(over="ignore"):
        return F32(1) / (F32(1) + np.exp2(F32(-L2E) * x))


def _fast_tanh(x):
    with np.errstate(over="ignore"):
        return F32(1) - F32(2) * (F32(1) / (F32(1) + np.exp2(F32(2 * L2E) * x)))


def emulate(whh: np.ndarray, xproj: np.ndarray, f16: bool, mutation: Optional[str] = None) -> np.ndarray:
    """What the kernels compute, in numpy: W (and, in the f16 mode, h) rounded to the element type, fp32 accumulation, the fast_*
    formulas, c carried in fp32 -> h [B][T][512] fp32.  `mutation` names one kernel bug (MUTATIONS):
        zero_fragment           one 16-unit x 32-k fragment of the candidate gate's W is dropped (units 80..95, k 192..223)
        swap_units              hidden units 37 and 150 read each other's W rows (all four gates)
        stale_h                 step T // 2 consumes the h of two steps before (a flipped buffer parity)
        reverse_walks_forward   direction 1 walks t = 0 .. T-1
        swap_f_i                the forget and input gates are exchanged
        scale_c                 c is scaled by 1 - C_EPS once, after step T // 2
    """
    assert mutation is None or mutation in MUTATIONS, mutation
    B, T = xproj.shape[:2]
    W = rounded(whh, f16).copy()
    x = xproj.astype(F32)
    if mutation == "zero_fragment":
        W[:, 2 * HID + 80:2 * HID + 96, 192:224] = 0
    if mutation == "swap_units":
        for gate in range(4):
            W[:, [gate * HID + 37, gate * HID + 150]] = W[:, [gate * HID + 150, gate * HID + 37]]
    out = np.zeros((B, T, 2 * HID), F32)
    for d in range(2):
        Wt = np.ascontiguousarray(W[d].T)
        zero = np.zeros((B, HID), F32)
        h, c, hist = zero, zero, []
        for s in range(T):
            t = s if (d == 0 or mutation == "reverse_walks_forward") else T - 1 - s
            hin = h
            if mutation == "stale_h" and s == T // 2:
                hin = hist[s - 2] if s >= 2 else zero
            pi, pf, pg, po = _gates((hin @ Wt).astype(F32) + x[:, t, d])
            if mutation == "swap_f_i":
                pi, pf = pf, pi
            c = _fast_sigmoid(pf) * c + _fast_sigmoid(pi) * _fast_tanh(pg)
            if mutation == "scale_c" and s == T // 2:
                c = c * F32(1.0 - C_EPS)
            h = rounded(_fast_sigmoid(po) * _fast_tanh(c), f16)
            hist.append(h)
            out[:, t, d * HID:(d + 1) * HID] = h
    return out


# ------------------------------------------------------------------------------------------------------------ operand sets
SAT_EVERY, CLIMB_EVERY = 37, 11

# B, T, gains, all-saturated xproj.  The smallest shapes at which the kernels can still go wrong:
GPU_CASES: Tuple[Tuple[int, int, Tuple[int, ...], bool], ...] = (
    (1, 1, (1, 3), False),      # the loop's flush never runs, only the final one; 15 masked rows
    (15, 2, (1, 3), False),     # first use of the second h buffer; ragged single tile
    (16, 3, (1, 3), False),     # exact tile; the buffer parity returns
    (17, 24, (1, 3), False),    # second workgroup with one live row; the CRNN length of a width-100 crop
    (33, 63, (1, 3), False),    # three workgroups; the production length; |c| about T
    (16, 63, (3,), True),       # every gate column at +-40
)


def case_params() -> List[Tuple[str, Dict[str, object]]]:
    """(id, make_case kwargs) of the GPU table, both gains"""
    return [(f"B{B}-T{T}-gain{gain}" + ("-saturated" if sat else ""), dict(B=B, T=T, gain=gain, saturated=sat))
            for B, T, gains, sat in GPU_CASES for gain in gains]


def make_case(B: int, T: int, gain: int, saturated: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """-> (whh [2][1024][256], xproj [B][T][2][1024]) fp32, seeded by the shape.
    W_hh uniform +-sqrt(3 / 256) gain: gain 1 is the recognizers' synthetic scale, gain 3 makes the recurrent term dominate.
    xproj uniform in +-2 with (a) every 37th gate column at +-40, the sign changing with the column, the row and every third
    step: sigmoids and tanh saturated in both signs;  (b) on every 11th unit forget = 9, input = 6, candidate = 5: c gains
    about 1 per step and |c| climbs to about T, past where exp2 overflows inside tanh(c) (c >= 44.4).
    saturated: every gate column at +-40, signs drawn at random."""
    rng = np.random.default_rng(100000 * gain + 1000 * B + 10 * T + int(saturated))
    whh = (rng.uniform(-1, 1, (2, 4 * HID, HID)) * math.sqrt(3.0 / HID) * gain).astype(F32)
    if saturated:
        return whh, (40.0 * rng.choice([-1.0, 1.0], (B, T, 2, 4 * HID))).astype(F32)
    x = rng.uniform(-2, 2, (B, T, 2, 4 * HID)).astype(F32)
    cols = np.arange(0, 4 * HID, SAT_EVERY)
    b, t = np.arange(B)[:, None, None], np.arange(T)[None, :, None]
    sign = 1.0 - 2.0 * ((cols[None, None, :] // SAT_EVERY + b + t // 3) % 2)
    x[:, :, :, cols] = (40.0 * sign)[:, :, None, :]
    units = np.arange(0, HID, CLIMB_EVERY)
    x[:, :, :, units] = 6.0
    x[:, :, :, HID + units] = 9.0
    x[:, :, :, 2 * HID + units] = 5.0
    return whh, x


def replace_rows(xproj: np.ndarray, first: int) -> np.ndarray:
    """xproj with rows first.. drawn anew (the row-independence check)"""
    rng = np.random.default_rng(77)
    out = xproj.copy()
    out[first:] = rng.uniform(-2, 2, out[first:].shape).astype(F32)
    return out
