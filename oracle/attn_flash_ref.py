"""ORACLE-SIDE TEST INFRASTRUCTURE (not product code) — the flash attention kernels of csrc/attn_flash.hip, plain and with
LayoutLMv3's relative-position bias and key mask, in fp64, with derived error bounds, a numpy emulation of the f16 kernel's
arithmetic, and the operand sets the kernel-level tests feed to ``mhip_attention_host``.

Reference.  Per (image, head, query) over the image's keys 0 .. n_keys - 1, from the operands the device received (all
f16-representable fp32, q already in the kernel's units):  s_j = q . k_j (+ T1[b(pj - pi)] + Tx[b(xj - xi)] + Ty[b(yj - yi)],
T = w * ATTN_SCORE_SCALE; a masked key: s_j = -inf),  p_j = 2^(s_j - max),  L = sum p_j >= 1,  ref = sum p_j v_j / L.

Bounds (``u16 = 2^-11``, ``u32 = 2^-24``; nothing below is taken from a run of the kernel).  Magnitudes, per element (query, head, d):
    A = sum p_j |v_j| / L,   B = sum p_j |v_j - ref| / L  (<= A + |ref|),   Brss = sqrt(sum p_j^2 (v_j - ref)^2) / L,
    V1 = sum_j |v_j - ref| / L  (all admitted keys, unweighted)
    smag = max_j (|q| . |k_j| + |T1| + |Tx| + |Ty|),   mmag = the largest |reference| the kernel can hold: max(|max of tile 0|, max_j |s_j|
           over the unmasked keys) — tile 0 sets the reference whatever it is (a wholly masked tile 0: about 1024), later a
           reference is always the maximum of a tile that exceeded the previous one, hence an unmasked score.
  f16 kernel (attn_flash_f16_kernel):
    score    an fp32 MFMA sum of 64 exact products started from -m, then (biased) three fp32 table adds of three fp32-rounded
             table entries, then (on a move) one subtraction:   ds = (64 + 2 [+ 6]) u32 (smag + mmag)    log2 units
    P        P' = f16(v_exp_f32(s')):  relative  rel = u16 + ln2 ds + 2^-21;  the SAME P' feeds numerator and denominator, so a
             relative error e_j of P_j moves the quotient by sum p_j e_j (v_j - ref) / L:  |.| <= rel B  (exactly: / (1 - rel)).
             A P below 2^-14 in the kernel's units is an f16 subnormal: absolute 2^-25 instead of u16.  The kernel's units are
             never smaller than the reference's (its m is some tile's maximum, <= max; later rescales multiply by alpha <= 1), and L
             >= 1, so that term is at most 2^-25 V1.
    sums     fp32 accumulation of n_keys terms in numerator and denominator, one rounding per rescale multiply (alpha itself
             is common to both and cancels), the reciprocal and the final product:  (n_keys + ntiles + 4) u32 (A + |ref|)
    store    f16:  u16 |ref| + 2^-25
    hard  = (rel B + 2^-25 V1) / (1 - rel) + (n_keys + ntiles + 4) u32 (A + |ref|) + u16 |ref| + 2^-25
    mean  = the same with sqrt(K) for each accumulation length K (64 + 2 [+ 6]; n_keys + ntiles + 4) and Brss for B in the u16
            term (the roundings of the P_j are independent); asserted as mean(err) <= mean(bound)
  fp32 kernel (attn_simple_f32_kernel): the same decomposition without the f16 terms and without a reference inside the score:
    ds32 = (64 + [6]) u32 smag + 2 u32 smag  (the fp32 sum; s - max),  rel32 = ln2 ds32 + 2^-21 (exp2f)
    sums: a lane's online loop of ceil(n_keys / 64) steps with three roundings each, a 6-step exchange tree, the final scale and
    division:  g32 = 3 ceil(n_keys / 64) + 12
    hard32 = rel32 B / (1 - rel32) + g32 u32 (A + |ref|) + u32 |ref| + 2^-126;   mean32: sqrt of both lengths

``emulate`` is the f16 kernel's arithmetic in numpy (64-key tiles in the kernel's key order, fp32 scores relative to the
reference, the reference set by tile 0 whatever it is, afterwards moved per query only on its own excess over 8 while the branch
is entered when any query of its 32-query wave exceeds, f16 P into both sums, f16 output); tests/test_oracle_attn_flash.py
asserts it within 1.0 of the hard bound on every case.  Variants ``no_branch`` / ``no_scaling`` serve the mutations.

Operands.  Every (image, head, query) has a target key — cycling through n_keys - 1, 0, 63 | 64, n_keys - 2, the first key of the
last tile, 31 | 32, 127 | 128 — and a query of noise plus a push along that key, so that boundary keys carry weight.  Rows a correct
kernel never admits hold 1.5 x the image's heaviest key: the padding rows n_keys .. npad_k - 1; where an image has none, row 0 of the
next image (an ordinary key there); behind the last image the slack.  The V^T columns of padding keys and the V^T slack hold 1000,
padding and slack query rows 24 with alternating signs, padding keys are NOT masked in the biased form (the kernel's own n_keys
test is what is pinned).  Everything is finite, as common.h requires.

``VARIANTS`` are softmax trajectories (see ``make_case``); ``assert_trajectory`` checks on the scores themselves that each one
happens.  ``mutations`` names likely kernel bugs as changes of the reference or of the emulation.

Block counts 7, 17 and 25 cannot be formed from heads 1 / 2 / 12 / 16, images 1 .. 3 and the query classes (1, 2, 3 or 5 blocks an
image): those three cases take 7, 17 and 5 heads.

Only ``tests/`` may import this module.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

U16, U32 = 2.0 ** -11, 2.0 ** -24
LN2 = math.log(2.0)
HD, TK, QB, WAVE = 64, 64, 128, 32
SLACK = 128                                   # ATTN_SLACK_ROWS
FUSED, SPLIT = 0, 1
SCALE_F32 = np.float32(0.125) * np.float32(1.4426950408889634)      # ATTN_SCORE_SCALE
MASKED = np.float32(-1024.0)                  # MHIP_ATTN_MASKED
RESCALE_AT = np.float32(8.0)
VARIANTS = ("tile0_max", "late_dominant", "rising", "identical", "shift_plus", "shift_minus", "shift_zero", "dip", "split_wave")
BIAS_VARIANTS = ("mask_first_tile", "mask_middle_tile", "mask_and_rescale")
T0, S0, SHIFT = 5, 12.0, 200.0
PAD_V, PAD_Q = 1000.0, 24.0
BINS_1D, MAX_1D, BINS_2D, MAX_2D = 32, 128, 64, 256
NOT_JUDGED: Dict[Tuple[str, str], str] = {}    # (case id, mutation) -> reason; empty: every applicable pair is judged


def f16(a) -> np.ndarray:
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def ceil8(n: int) -> int:
    return (n + 7) // 8 * 8


def ntiles(n_keys: int) -> int:
    return (n_keys + TK - 1) // TK


def nqb(n_queries: int) -> int:
    return (n_queries + QB - 1) // QB


def tile_key_order() -> np.ndarray:
    """key of LDS row R = 16 kt + i of a tile: 32 (kt >> 1) + 8 (i >> 2) + 4 (kt & 1) + (i & 3)  (attn_flash.hip, restated)"""
    R = np.arange(TK)
    kt, i = R >> 4, R & 15
    return 32 * (kt >> 1) + 8 * (i >> 2) + 4 * (kt & 1) + (i & 3)


def xcd_remap(bid: int, nblk: int) -> int:
    """logical block of hardware block `bid` among nblk (attn_flash.hip, restated)"""
    q, r, xcd = nblk >> 3, nblk & 7, bid & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


# ---------------------------------------------------------------------------------------------------------------- operands
def target_cycle(n_keys: int) -> List[int]:
    cands = [n_keys - 1, 0, 63, 64, n_keys - 2, (ntiles(n_keys) - 1) * TK, 31, 32, 127, 128]
    out: List[int] = []
    for k in cands:
        if 0 <= k < n_keys and k not in out:
            out.append(k)
    return out


def make_case(images: int, heads: int, n_queries: int, n_keys: int, npad_q: int, npad_k: int, layout: int = SPLIT,
              variant: Optional[str] = None, bias: Optional[dict] = None, seed: int = 0, rise: bool = True) -> Dict[str, object]:
    """operands of one call.  q [images * npad_q + SLACK][D], k [images * npad_k + SLACK][D], vt [D * images * npad_k + SLACK]
    (V^T flat, then its slack); with ``bias`` = dict(dp, dx, masks): qcode [rows][3], kcode [rows][4], w1 / wx / wy.

    variants (every (query, head) targets key 5 with a q . k of exactly 12 log2 units, noise orthogonal to the push):
      tile0_max      nothing else: tile 0 holds the global maximum, the reference never moves
      late_dominant  the last key is 3 x key 5: 24 above everything before it, one rescale in the last tile
      rising         keys 69, 133, 197 are (1 + 7 i / 12) x key 5: tile maxima 12, 19, 26, 33 — no move at +7, one at +14, P of 2^7
      identical      every key of an image is the image's row 0
      shift_plus / shift_minus / shift_zero   late_dominant with component 63 of every key 1 and of every query +200 / -200 / 0
      dip            every key from 64 on is -1.5 x key 5 plus a little noise: 30 below tile 0, P underflows f16
      split_wave     key 133 scores 32 for the odd queries (a move in tile 2; without it P = 2^20 leaves f16) and 0 for the even
                     ones (none); rise=False: 0 for all
    bias["masks"]: per image one of "none", "random" (40 % masked), "first_tile", "middle_tile" (keys 64 .. 127); the target keys
    and the last key stay valid."""
    assert variant is None or variant in VARIANTS
    assert n_queries <= npad_q and n_keys <= npad_k and npad_k % 8 == 0 and (layout == SPLIT or npad_q == npad_k)
    rng = np.random.default_rng(seed)
    D = heads * HD
    K = f16(rng.normal(0, 1.0, (images, npad_k, heads, HD)))
    V = f16(rng.normal(0, 1.0, (images, npad_k, heads, HD)))
    shift = variant in ("shift_plus", "shift_minus", "shift_zero")
    if variant is None:
        cyc = target_cycle(n_keys)
        tgt = np.array([[[cyc[((i * heads + h) * 3 + r) % len(cyc)] for r in range(n_queries)] for h in range(heads)]
                        for i in range(images)], np.int64)
        top = [int(tgt[i, 0, 0]) for i in range(images)]
    else:
        assert n_keys >= 4 * TK + 1
        tgt = np.full((images, heads, n_queries), T0, np.int64)
        top = [T0] * images
        if variant == "identical":
            K[:, :n_keys] = K[:, :1]
        elif variant == "rising":
            for i in (1, 2, 3):
                K[:, TK * i + T0] = f16((1.0 + 7.0 * i / S0) * K[:, T0])
            top = [3 * TK + T0] * images
        elif variant == "dip":
            K[:, TK:n_keys] = f16(-1.5 * K[:, T0:T0 + 1] + 0.3 * K[:, TK:n_keys])
        elif variant in ("late_dominant",) or shift:
            K[:, n_keys - 1] = f16(3.0 * K[:, T0])
            top = [n_keys - 1] * images
    if shift:
        K[..., HD - 1] = 1.0
    for i in range(images):
        heavy = f16(1.5 * K[i, top[i]])
        if npad_k > n_keys:
            K[i, n_keys:] = heavy
            V[i, n_keys:] = PAD_V
        elif i + 1 < images:
            K[i + 1, 0] = heavy
    k_slack = np.broadcast_to(f16(1.5 * K[images - 1, top[images - 1]]).reshape(1, D), (SLACK, D)).copy()
    if shift:                        # the heavy rows take the same shift as every key
        for i in range(images):
            K[i, n_keys:, :, HD - 1] = 1.0
            if npad_k == n_keys and i + 1 < images:
                K[i + 1, 0, :, HD - 1] = 1.0
        k_slack[:, HD - 1::HD] = 1.0
    # queries: noise + push along the target key (log2 units)
    K64 = K.astype(np.float64)
    kt = K64[np.arange(images)[:, None, None], tgt, np.arange(heads)[None, :, None]]          # [images][heads][nq][64]
    if variant is None:
        # noise scores N(0, 1.6) log2 units against the keys (mean weight about 1.8 each): a push of log2(2 n) + 1 puts about
        # half of the weight on the target
        push = max(4.0, math.log2(2.0 * n_keys) + 1.0)
        q = rng.normal(0, 0.2, kt.shape) + push * kt / (kt * kt).sum(-1, keepdims=True)
    else:
        noise = rng.normal(0, 0.06, kt.shape)
        basis = [kt.copy()]
        if shift:
            basis[0][..., HD - 1] = 0.0
            noise[..., HD - 1] = 0.0
        b0 = basis[0]
        n0 = (b0 * b0).sum(-1, keepdims=True)
        noise -= (noise * b0).sum(-1, keepdims=True) / n0 * b0
        q = noise + S0 * b0 / n0
        if variant == "split_wave":
            r = K64[:, 2 * TK + T0].reshape(images, heads, 1, HD)                            # key 133, a fresh random row
            rp = r - (r * b0).sum(-1, keepdims=True) / n0 * b0
            nr = (rp * rp).sum(-1, keepdims=True)
            q -= (noise * rp).sum(-1, keepdims=True) / nr * rp
            cross = S0 * (b0 * r).sum(-1, keepdims=True) / n0                               # what the push alone scores on key 133
            odd = (np.arange(n_queries) % 2 == 1).reshape(1, 1, -1, 1)
            beta = np.where(odd & rise, 32.0, 0.0) - cross
            q = q + beta * rp / nr
        if shift:
            q[..., HD - 1] = {"shift_plus": SHIFT, "shift_minus": -SHIFT, "shift_zero": 0.0}[variant]
    sign = np.where(np.arange(D) % 2 == 0, PAD_Q, -PAD_Q).astype(np.float32)
    Q = np.empty((images, npad_q, D), np.float32)
    Q[:] = sign
    Q[:, :n_queries] = f16(np.transpose(q, (0, 2, 1, 3)).reshape(images, n_queries, D))
    qf = np.concatenate([Q.reshape(-1, D), np.broadcast_to(sign, (SLACK, D))]).astype(np.float32)
    kf = np.concatenate([K.reshape(-1, D), k_slack]).astype(np.float32)
    vt = np.concatenate([np.transpose(V, (2, 3, 0, 1)).reshape(-1), np.full(SLACK, PAD_V, np.float32)]).astype(np.float32)
    case = {"images": images, "heads": heads, "n_queries": n_queries, "n_keys": n_keys, "npad_q": npad_q, "npad_k": npad_k,
            "layout": layout, "variant": variant, "q": qf, "k": kf, "vt": vt, "targets": tgt, "bias": None}
    if bias is not None:
        dp, dx = bias["dp"], bias["dx"]
        rq, rk = qf.shape[0], kf.shape[0]
        pos_k, x_k, y_k = rng.integers(0, dp + 1, rk), rng.integers(0, dx + 1, rk), rng.integers(0, dx + 1, rk)
        if layout == FUSED:          # self-attention rows: a token is one row as query and as key
            pos_q, x_q, y_q = pos_k, x_k, y_k
        else:
            pos_q, x_q, y_q = rng.integers(0, dp + 1, rq), rng.integers(0, dx + 1, rq), rng.integers(0, dx + 1, rq)
        valid = np.ones(rk, np.int32)
        for i, m in enumerate(bias["masks"][j % len(bias["masks"])] for j in range(images)):
            v = valid[i * npad_k:i * npad_k + n_keys]
            if m == "random":
                v[rng.random(n_keys) < 0.4] = 0
            elif m == "first_tile":
                v[:TK] = 0
            elif m == "middle_tile":
                v[TK:2 * TK] = 0
            else:
                assert m == "none"
            if m != "none":
                keep = set(tgt[i].ravel().tolist()) | {n_keys - 1}
                if m == "first_tile":
                    keep = {k for k in keep if k >= TK} | {n_keys - 1}
                elif m == "middle_tile":
                    keep = {k for k in keep if not TK <= k < 2 * TK}
                v[sorted(keep)] = 1
        case["bias"] = {"dp": dp, "dx": dx, "max_1d": MAX_1D, "max_2d": MAX_2D,
                        "qcode": np.stack([pos_q, x_q, y_q], 1).astype(np.int32),
                        "kcode": np.stack([pos_k, x_k, y_k, valid], 1).astype(np.int32),
                        "w1": rng.uniform(-4, 4, (heads, BINS_1D)).astype(np.float32),
                        "wx": rng.uniform(-4, 4, (heads, BINS_2D)).astype(np.float32),
                        "wy": rng.uniform(-4, 4, (heads, BINS_2D)).astype(np.float32)}
    return case


# -------------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def _buckets(bins: int, maxd: int, dmax: int) -> np.ndarray:
    """bucket of every difference -dmax .. dmax (tests/layoutlmv3_ref.relative_position_bucket)"""
    import torch
    from layoutlmv3_ref import relative_position_bucket

    return relative_position_bucket(torch.arange(-dmax, dmax + 1), bins, maxd).numpy()


def bias_tables(case, drop: Optional[str] = None):
    """per head the three difference-indexed tables in fp64 from the fp32 weights and the fp32 scale: t1 [heads][2 dp + 1], tx,
    ty [heads][2 dx + 1].  drop: "p" / "x" / "y" zeroes that field's table (a mutation)."""
    b = case["bias"]
    s = float(SCALE_F32)
    t1 = b["w1"].astype(np.float64)[:, _buckets(BINS_1D, b["max_1d"], b["dp"])] * s
    tx = b["wx"].astype(np.float64)[:, _buckets(BINS_2D, b["max_2d"], b["dx"])] * s
    ty = b["wy"].astype(np.float64)[:, _buckets(BINS_2D, b["max_2d"], b["dx"])] * s
    if drop == "p":
        t1 = t1 * 0
    if drop == "x":
        tx = tx * 0
    if drop == "y":
        ty = ty * 0
    return t1, tx, ty


def gather(case, img: int, keys: np.ndarray, kv_img: Optional[int] = None):
    """(K rows [S][heads][64], V rows [S][heads][64], flat key rows) at the addresses the kernel forms: key row
    img * npad_k + key of k, column img * npad_k + key of row d of V^T — past an image they run on into the next one / the slack"""
    heads, ldv = case["heads"], case["images"] * case["npad_k"]
    rows = (img if kv_img is None else kv_img) * case["npad_k"] + np.asarray(keys)
    Kr = case["k"][rows].reshape(len(rows), heads, HD)
    col = np.arange(heads * HD)[None, :] * ldv + rows[:, None]
    Vr = case["vt"][col].reshape(len(rows), heads, HD)
    return Kr, Vr, rows


def bias_scores(case, img: int, rows_k: np.ndarray, tabs, use_mask: bool = True):
    """(bias [heads][nq][S] fp64, |.| summed the same way, masked [S] bool) for the image's queries against flat key rows"""
    b = case["bias"]
    nq, dp, dx = case["n_queries"], b["dp"], b["dx"]
    qc = b["qcode"][img * case["npad_q"]:img * case["npad_q"] + nq].astype(np.int64)
    kc = b["kcode"][rows_k].astype(np.int64)
    t1, tx, ty = tabs
    ip = kc[None, :, 0] - qc[:, None, 0] + dp
    ix = kc[None, :, 1] - qc[:, None, 1] + dx
    iy = kc[None, :, 2] - qc[:, None, 2] + dx
    bs = t1[:, ip] + tx[:, ix] + ty[:, iy]
    ba = np.abs(t1[:, ip]) + np.abs(tx[:, ix]) + np.abs(ty[:, iy])
    masked = (kc[:, 3] == 0) if use_mask else np.zeros(len(rows_k), bool)
    return bs, ba, masked


def reference(case, keys=None, kv_img: Optional[int] = None, drop: Optional[str] = None, use_mask: bool = True,
              prec16: bool = True, bounds: bool = True) -> Dict[str, np.ndarray]:
    """softmax2 attention in fp64 with the hard and the mean bound of the f16 (prec16) or the fp32 kernel (both are always there
    as hard / mean and hard32 / mean32; prec16 = False puts the fp32 kernel's under hard / mean).
    keys: the keys of an image attended (default 0 .. n_keys - 1); kv_img: every image reads this image's K / V (a mutation).
    -> ref, hard, mean [images][n_queries][heads * 64]; scores, p [images][heads][n_queries][S]"""
    images, heads, nq, n, npq = (case[k] for k in ("images", "heads", "n_queries", "n_keys", "npad_q"))
    keys = np.arange(n) if keys is None else np.asarray(keys)
    S = len(keys)
    out = {k: np.empty((images, nq, heads, HD)) for k in ("ref", "hard", "mean", "hard32", "mean32")}
    out["scores"] = np.empty((images, heads, nq, S))
    out["p"] = np.empty((images, heads, nq, S))
    tabs = bias_tables(case, drop) if case["bias"] is not None else None
    nb = 6 if tabs is not None else 0
    for i in range(images):
        Kr, Vr, rows = gather(case, i, keys, kv_img)
        K64, V64 = Kr.astype(np.float64), Vr.astype(np.float64)
        Q64 = case["q"][i * npq:i * npq + nq].astype(np.float64).reshape(nq, heads, HD)
        s = np.einsum("qhd,shd->hqs", Q64, K64)
        sa = np.einsum("qhd,shd->hqs", np.abs(Q64), np.abs(K64))
        full = s
        masked = np.zeros(S, bool)
        if tabs is not None:
            bs, ba, masked = bias_scores(case, i, rows, tabs, use_mask)
            s = s + bs
            sa = sa + ba
            full = np.where(masked[None, None, :], s + float(MASKED), s)
            s = np.where(masked[None, None, :], -np.inf, s)
        assert not masked.all(), "an image with every key masked has no reference"
        smag = sa.max(-1)                                                        # [heads][nq]
        mmag = np.maximum(np.abs(full[..., :TK].max(-1)), np.abs(np.where(masked, 0.0, s)).max(-1))
        p = np.exp2(s - s.max(-1, keepdims=True))
        L = p.sum(-1, keepdims=True)
        pn = p / L
        ref = np.einsum("hqs,shd->qhd", pn, V64)
        out["ref"][i] = ref
        out["scores"][i] = s
        out["p"][i] = pn
        if not bounds:
            continue
        A = np.einsum("hqs,shd->qhd", pn, np.abs(V64))
        B, Brss, V1 = np.empty_like(ref), np.empty_like(ref), np.empty_like(ref)
        for h in range(heads):                                                   # |v_j - ref| is [nq][S][64]: in slices
            for c0 in range(0, nq, 64):
                sl = slice(c0, min(nq, c0 + 64))
                dev = np.abs(V64[None, :, h] - ref[sl, None, h])
                w = pn[h, sl, :, None]
                B[sl, h] = (w * dev).sum(1)
                Brss[sl, h] = np.sqrt((w * w * dev * dev).sum(1))
                V1[sl, h] = (dev * (~masked)[None, :, None]).sum(1) / L[h, sl]
        aref = np.abs(ref)
        sm, mm = smag.T[..., None], mmag.T[..., None]                            # [nq][heads][1]
        nt, na = HD + 2 + nb, n + ntiles(n) + 4
        for name, kt_, ka_, Bp in (("hard", nt, na, B), ("mean", math.sqrt(nt), math.sqrt(na), Brss)):
            ds = kt_ * U32 * (sm + mm)
            rel_s = LN2 * ds + 2.0 ** -21
            rel = U16 + rel_s
            out[name][i] = ((U16 * Bp + rel_s * B + 2.0 ** -25 * V1) / (1 - rel) + ka_ * U32 * (A + aref) + U16 * aref + 2.0 ** -25)
        nt, na = HD + nb, 3 * ntiles(n) + 12
        for name, kt_, ka_ in (("hard32", nt, na), ("mean32", math.sqrt(nt), math.sqrt(na))):
            rel = LN2 * (kt_ + 2) * U32 * sm + 2.0 ** -21
            out[name][i] = rel * B / (1 - rel) + ka_ * U32 * (A + aref) + U32 * aref + 2.0 ** -126
    for k in ("ref", "hard", "mean", "hard32", "mean32"):
        out[k] = out[k].reshape(images, nq, heads * HD)
    if not prec16:
        out["hard"], out["mean"] = out["hard32"], out["mean32"]
    return out


def judged_rows(case, out: np.ndarray) -> np.ndarray:
    """rows < n_queries of every image of the device's whole output [images * npad_q + SLACK][D] -> [images][n_queries][D]"""
    images, nq, npq = case["images"], case["n_queries"], case["npad_q"]
    return np.asarray(out)[:images * npq].reshape(images, npq, -1)[:, :nq]


# --------------------------------------------------------------------------------------------------------------- emulation
def emulate(case, rescale: str = "kernel", info: bool = False):
    """the f16 kernel's arithmetic in numpy -> [images][n_queries][D] fp32 (f16 values); info: which (image, head, query, tile)
    moved its reference, which (image, wave, tile) entered the branch, log2 of the largest P per (image, head, query, tile).
    rescale: "kernel"; "no_branch" (after tile 0 the reference never moves); "no_scaling" (it moves, the sums are not scaled)"""
    images, heads, nq, n, npq, npk = (case[k] for k in ("images", "heads", "n_queries", "n_keys", "npad_q", "npad_k"))
    nt, order = ntiles(n), tile_key_order()
    nwave = nqb(nq) * QB // WAVE
    out = np.full((images, nqb(nq) * QB, heads, HD), np.nan, np.float32)
    moved = np.zeros((images, heads, nwave * WAVE, nt), bool)
    branch = np.zeros((images, heads, nwave, nt), bool)
    pmax = np.zeros((images, heads, nwave * WAVE, nt))
    tabs32 = None
    if case["bias"] is not None:
        b = case["bias"]
        t1, tx, ty = (t.astype(np.float32) for t in bias_tables(case))
        t1 = np.concatenate([t1, np.full((heads, b["dp"] + 1), MASKED, np.float32)], 1)      # entries 2 dp + 1 .. 3 dp + 1
        tabs32 = (t1, tx, ty)
    with np.errstate(all="ignore"):
        for i in range(images):
            for w in range(nwave):
                r0 = i * npq + w * WAVE
                Q = case["q"][r0:r0 + WAVE].reshape(WAVE, heads, HD)
                acc = np.zeros((heads, WAVE, HD), np.float32)
                lsum = np.zeros((heads, WAVE), np.float32)
                negm = np.zeros((heads, WAVE), np.float32)
                for t in range(nt):
                    keys = t * TK + order
                    Kr, Vr, rows = gather(case, i, keys)
                    s = (np.einsum("qhd,shd->hqs", Q, Kr).astype(np.float32) + negm[..., None]).astype(np.float32)
                    if tabs32 is not None:
                        qc = case["bias"]["qcode"][r0:r0 + WAVE].astype(np.int64)
                        kc = case["bias"]["kcode"][rows].astype(np.int64)
                        kp = np.where(kc[:, 3] != 0, kc[:, 0], 2 * case["bias"]["dp"] + 1)
                        ip = kp[None, :] - qc[:, None, 0] + case["bias"]["dp"]
                        ix = kc[None, :, 1] - qc[:, None, 1] + case["bias"]["dx"]
                        iy = kc[None, :, 2] - qc[:, None, 2] + case["bias"]["dx"]
                        s = s + ((tabs32[0][:, ip] + tabs32[1][:, ix]) + tabs32[2][:, iy])
                    s[..., keys >= n] = -np.inf
                    tmax = s.max(-1)
                    if t == 0:
                        mv = np.ones_like(tmax, bool)
                        d, alpha = tmax, np.zeros_like(tmax)
                        enter = True
                    else:
                        mv = tmax > RESCALE_AT
                        d = np.where(mv, tmax, np.float32(0))
                        alpha = np.exp2(-d)
                        enter = mv.any(1) if rescale != "no_branch" else np.zeros(heads, bool)
                        mv = mv & np.asarray(enter)[:, None]
                    e = np.broadcast_to(np.asarray(enter).reshape(-1, 1), tmax.shape)
                    d = np.where(e, d, np.float32(0)).astype(np.float32)
                    negm = (negm - d).astype(np.float32)
                    s = (s - d[..., None]).astype(np.float32)
                    if rescale != "no_scaling" or t == 0:
                        a = np.where(e, alpha, np.float32(1)).astype(np.float32)
                        lsum = lsum * a
                        acc = acc * a[..., None]
                    p = f16(np.exp2(s))
                    lsum = (lsum + p.sum(-1, dtype=np.float32)).astype(np.float32)
                    acc = (acc + np.einsum("hqs,shd->hqd", p, Vr).astype(np.float32)).astype(np.float32)
                    moved[i, :, w * WAVE:(w + 1) * WAVE, t] = mv
                    branch[i, :, w, t] = enter
                    pmax[i, :, w * WAVE:(w + 1) * WAVE, t] = s.max(-1)
                o = f16(acc * (np.float32(1) / lsum)[..., None])
                out[i, w * WAVE:(w + 1) * WAVE] = np.transpose(o, (1, 0, 2))
    res = out[:, :nq].reshape(images, nq, heads * HD)
    if info:
        return res, {"moved": moved[:, :, :nq], "branch": branch, "log2_pmax": pmax[:, :, :nq]}
    return res


def assert_trajectory(case) -> None:
    """the variant's softmax trajectory happens, judged on the scores of the reference"""
    v, n, nq = case["variant"], case["n_keys"], case["n_queries"]
    if v is None:
        return
    c = reference(case)
    s = c["scores"]                                                                       # [images][heads][nq][n]
    nt = ntiles(n)
    tmax = np.stack([s[..., t * TK:(t + 1) * TK].max(-1) for t in range(nt)], -1)         # [images][heads][nq][ntiles]
    _, inf = emulate(case, info=True)
    mv = inf["moved"]
    if v == "identical":
        assert np.ptp(s, axis=-1).max() <= 1e-9 * max(1.0, np.abs(s).max()), "identical keys, identical scores"
        return
    if v == "tile0_max":
        assert (tmax[..., 0:1] >= tmax).all() and not mv[..., 1:].any()
        return
    if v == "dip":
        assert (tmax[..., 1:].max(-1) < tmax[..., 0] - 24.0).all(), "every later tile more than 24 below tile 0"
        assert not mv[..., 1:].any() and (inf["log2_pmax"][..., 1:] < -24.0).all(), "P underflows f16 in every later tile"
        return
    if v == "rising":
        step = np.diff(tmax[..., :4], axis=-1)
        assert (np.abs(step - 7.0) <= 0.5).all(), "tile maxima rise by about 7 log2 units over the first four tiles"
        assert not mv[..., 1].any() and mv[..., 2].all() and not mv[..., 3:].any()
        assert (inf["log2_pmax"][..., 1] >= 6.5).all() and (inf["log2_pmax"][..., 3] >= 6.5).all() and inf["log2_pmax"].max() <= 8.0
        return
    if v == "split_wave":
        odd = np.arange(nq) % 2 == 1
        assert (np.abs(tmax[:, :, odd, 2] - tmax[:, :, odd, 0] - 20.0) <= 0.5).all(), "odd queries: tile 2 is 20 above tile 0"
        assert (tmax[:, :, ~odd, 1:].max(-1) <= tmax[:, :, ~odd, 0]).all(), "even queries: tile 0 holds the maximum"
        assert mv[:, :, odd, 2].all() and not mv[:, :, ~odd, 1:].any() and not mv[:, :, odd, 1].any() and not mv[:, :, odd, 3:].any()
        assert inf["branch"][:, :, :(nq + WAVE - 1) // WAVE, 2].all(), "the wave enters the branch in tile 2 for the even queries too"
        return
    # late_dominant and the shifts: the last tile outgrows everything before it by more than 16 (without the rescale P would
    # leave the f16 range)
    lead = tmax[..., -1] - tmax[..., :-1].max(-1)
    assert (lead >= 20.0).all() and mv[..., -1].all() and not mv[..., 1:-1].any()
    if v in ("shift_plus", "shift_minus"):
        sign = 1.0 if v == "shift_plus" else -1.0
        assert (sign * s[..., :n - 1] >= SHIFT - 16.0).all() and (sign * s[..., :n - 1] <= SHIFT + 16.0).all()


def assert_bias_trajectory(case, kind: str) -> None:
    """the biased cases' promises, on the mask and on the emulation's reference moves"""
    n, npk = case["n_keys"], case["npad_k"]
    valid = case["bias"]["kcode"][:case["images"] * npk, 3].reshape(case["images"], npk)[:, :n]
    _, inf = emulate(case, info=True)
    if kind == "mask_first_tile":
        assert (valid[:, :TK] == 0).all(axis=1).any() and inf["moved"][np.where((valid[:, :TK] == 0).all(axis=1))[0]][..., 1].all()
    elif kind == "mask_middle_tile":
        hit = (valid[:, TK:2 * TK] == 0).all(axis=1)
        assert hit.any() and (valid[hit][:, :TK] == 1).any() and (valid[hit][:, 2 * TK:] == 1).any()
    else:
        assert (valid == 0).any(axis=1).all() and inf["moved"][..., -1].all(), "masked keys in images that rescale in the last tile"


# --------------------------------------------------------------------------------------------------------------- mutations
def mutations(case) -> Dict[str, np.ndarray]:
    """name -> [images][n_queries][D] under that kernel bug, for the bugs that apply to the case.  Dropping a key applies where
    some query targets it (in the variants: the dominant last key only)."""
    images, heads, nq, n, npk = (case[k] for k in ("images", "heads", "n_queries", "n_keys", "npad_k"))
    v = case["variant"]
    ref = reference(case, bounds=False)["ref"]
    tg = set(case["targets"].ravel().tolist()) if v is None else ({n - 1} if v == "late_dominant" or v.startswith("shift") else set())
    if case["bias"] is not None:                  # a masked key's absence is no bug
        valid = case["bias"]["kcode"][:images * npk, 3].reshape(images, npk)[:, :n]
        tg = {k for k in tg if valid[:, k].all()}
    out: Dict[str, np.ndarray] = {}
    keys = np.arange(n)
    if n >= 2:
        for name, k in (("drop_last_key", n - 1), ("drop_first_key", 0), ("drop_key_63", 63), ("drop_key_64", 64)):
            if k in tg:
                out[name] = reference(case, keys=keys[keys != k], bounds=False)["ref"]
    out["admit_key_n"] = reference(case, keys=np.arange(n + 1), bounds=False)["ref"]
    if images >= 2:
        out["image0_kv_for_all"] = reference(case, kv_img=0, bounds=False)["ref"]
    if heads >= 2:
        sw = ref.reshape(images, nq, heads, HD).copy()
        sw[:, :, [0, 1]] = sw[:, :, [1, 0]]
        out["swap_heads_0_1"] = sw.reshape(ref.shape)
    if nq >= 32 and n >= 2 and v in (None, "split_wave"):
        sw = ref.copy()
        full = nq // 32 * 32
        blk = sw[:, :full].reshape(images, full // 32, 2, 16, -1)
        sw[:, :full] = blk[:, :, ::-1].reshape(images, full, -1)
        out["swap_query_tiles"] = sw
    bias_late = case["bias"] is not None and case.get("bias_kind") == "mask_and_rescale"
    if v in ("late_dominant", "rising", "shift_plus", "shift_minus", "shift_zero", "split_wave") or bias_late:
        out["no_branch"] = emulate(case, rescale="no_branch").astype(np.float64)
        out["no_scaling"] = emulate(case, rescale="no_scaling").astype(np.float64)
    if case["bias"] is not None and v is None:      # in a variant one key holds all the weight: the bias cannot show
        for f in ("p", "x", "y"):
            out[f"bias_table_{f}_dropped"] = reference(case, drop=f, bounds=False)["ref"]
        if (case["bias"]["kcode"][:images * npk, 3].reshape(images, npk)[:, :n] == 0).any():
            out["mask_ignored"] = reference(case, use_mask=False, bounds=False)["ref"]
    return out


def moved(mut: np.ndarray, ref: np.ndarray, bound: np.ndarray) -> float:
    """the largest |mut - ref| / bound over the elements; a non-finite result counts as infinitely far"""
    if not np.isfinite(mut).all():
        return math.inf
    return float((np.abs(mut - ref) / bound).max())


# -------------------------------------------------------------------------------------------------------------- case tables
N_KEYS = (1, 8, 63, 64, 65, 128, 129, 193, 577)
N_QUERIES = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)
HEADS = (1, 2, 12, 16)
BLOCK_COUNTS = (1, 3, 7, 8, 9, 15, 17, 25)
VARIANT_SHAPE = dict(images=2, heads=2, n_queries=40, n_keys=4 * TK + 9)          # five tiles, two waves (one partial), padding rows


def _kw(layout, images, heads, nq, nk, xq, xk, variant=None, bias=None, bias_kind=None):
    npq, npk = ceil8(nq) + xq, ceil8(nk) + xk
    if layout == FUSED:
        npq = npk = max(npq, npk)
    vid = f"-{variant}" if variant else ""
    bid = "" if bias is None else f"-b{bias['dp']}x{bias['dx']}" + (f"-{bias_kind}" if bias_kind else "")
    vi = 0 if variant is None else 1 + VARIANTS.index("shift_plus" if variant.startswith("shift") else variant)   # the shifts share operands
    seed = layout + images * 3 + heads * 31 + nq * 1009 + nk * 13 + xq * 5 + xk * 7 + vi * 100003 + (0 if bias is None else 17 + bias["dp"])
    kw = dict(images=images, heads=heads, n_queries=nq, n_keys=nk, npad_q=npq, npad_k=npk, layout=layout, variant=variant,
              bias=bias, seed=seed)
    return (f"{'fused' if layout == FUSED else 'split'}-i{images}-h{heads}-q{nq}of{npq}-k{nk}of{npk}{vid}{bid}", kw)


def sweep_params():
    """every n_keys class and every n_queries class in both layouts; heads, images and the pitches rotated through the table"""
    out = []
    # fused: self-attention (n_queries == n_keys) over the key classes, and query classes below a larger key count
    for ki, n in enumerate(N_KEYS):
        heads, images, x = HEADS[ki % 4], 1 + ki % 3, 8 * (ki % 2)
        if n >= 193:
            heads, images = 2, 2
        if images == 1 and x == 0 and n % 8 == 0:
            images = 2                          # no padding rows: the row behind the last key is the next image's
        out.append(_kw(FUSED, images, heads, n, n, x, x))
    for qi, nq in enumerate(N_QUERIES):
        nk = N_KEYS[(qi + 3) % len(N_KEYS)]
        heads, images, x = HEADS[(qi + 1) % 4], 1 + (qi + 1) % 3, 8 * ((qi + 1) % 2)
        if nq >= 127 and heads > 2:
            heads = 2
        if nk == 577:
            heads, images = min(heads, 2), min(images, 2)
        if nq > ceil8(nk) + x:                  # a fused launch has one pitch: the queries must fit into the key rows
            nk, heads, images = (193 if nq <= 193 else 577), min(heads, 2), min(images, 2)
        out.append(_kw(FUSED, images, heads, nq, nk, x, x))
        nk2 = N_KEYS[(qi + 6) % len(N_KEYS)]
        out.append(_kw(SPLIT, 1 + qi % 3, heads, nq, 65 if nk2 == 577 else nk2, 8 * (qi % 2), 8 * ((qi // 2) % 2)))
    for ki, n in enumerate(N_KEYS):
        nq = N_QUERIES[(2 * ki + 1) % len(N_QUERIES)]
        heads, images = HEADS[(ki + 2) % 4], 1 + (ki + 1) % 3
        if n == 577 or nq >= 127:
            heads, images = min(heads, 2), min(images, 2)
        out.append(_kw(SPLIT, images, heads, nq, n, 8 * ((ki + 1) % 2), 8 * (ki % 2)))
    out.append(_kw(SPLIT, 2, 2, 100, 65, 264 - 104, 0))          # npad_q 264 far above n_queries 100
    # block counts nqb * heads * images
    out += [_kw(SPLIT, 1, 1, 17, 65, 0, 8),                        # 1
            _kw(SPLIT, 1, 1, 257, 65, 8, 0),                       # 3
            _kw(FUSED, 1, 7, 63, 63, 0, 0),                        # 7: below 8, every block on an XCD of its own
            _kw(SPLIT, 2, 2, 129, 64, 0, 0),                       # 8
            _kw(SPLIT, 3, 1, 257, 8, 0, 8),                        # 9
            _kw(FUSED, 3, 1, 577, 577, 0, 0),                      # 15
            _kw(FUSED, 1, 17, 33, 65, 0, 0),                       # 17
            _kw(SPLIT, 1, 5, 577, 63, 0, 0)]                       # 25
    seen, uniq = set(), []
    for pid, kw in out:
        if pid not in seen:
            seen.add(pid)
            uniq.append((pid, kw))
    return uniq


def variant_params():
    """each trajectory on one two-image, two-head shape of five tiles, fused layout"""
    s = VARIANT_SHAPE
    return [_kw(FUSED, s["images"], s["heads"], s["n_queries"], s["n_keys"], 0, 0, v) for v in VARIANTS]


def bias_params():
    """the biased form: n 65 / 197 / 264, images 2 and 3 with a different mask per image, dp / dx small and the product's 511 / 1000"""
    small, prod = dict(dp=7, dx=9), dict(dp=511, dx=1000)
    out = []
    for (n, images, heads, layout, x), b, masks, kind in (
            ((65, 2, 12, FUSED, 0), small, ("none", "random"), None),
            ((65, 3, 1, SPLIT, 8), prod, ("random", "none", "random"), None),
            ((197, 2, 2, FUSED, 0), prod, ("first_tile", "random"), "mask_first_tile"),
            ((197, 3, 2, FUSED, 8), small, ("random", "middle_tile", "none"), "mask_middle_tile"),
            ((264, 2, 2, FUSED, 0), prod, ("middle_tile", "first_tile"), "mask_middle_tile"),
            ((264, 3, 1, SPLIT, 0), small, ("first_tile", "none", "random"), "mask_first_tile")):
        out.append(_kw(layout, images, heads, n, n, x, x, None, dict(b, masks=masks), kind))
    s = VARIANT_SHAPE
    out.append(_kw(FUSED, 3, 2, s["n_queries"], s["n_keys"], 0, 0, "late_dominant", dict(prod, masks=("random", "random", "random")),
                   "mask_and_rescale"))
    return out


def all_params():
    return sweep_params() + variant_params() + bias_params()


def build(pid_kw) -> Dict[str, object]:
    """the case of one (id, kw) entry of the tables"""
    pid, kw = pid_kw
    case = make_case(**kw)
    case["id"] = pid
    case["bias_kind"] = pid.rsplit("-", 1)[1] if pid.rsplit("-", 1)[1] in BIAS_VARIANTS else None
    return case


def isolation_params():
    """shapes for the bit-for-bit isolation checks: three images without and with padding rows, several heads, more than two tiles"""
    return [_kw(FUSED, 3, 2, 129, 129, 0, 0), _kw(FUSED, 2, 12, 64, 64, 0, 0), _kw(SPLIT, 3, 2, 33, 193, 8, 8),
            _kw(FUSED, 2, 2, 197, 197, 0, 0, None, dict(dp=511, dx=1000, masks=("random", "first_tile")))]


# ------------------------------------------------------------------------------------------------ derived cases (isolation)
def _derive(case, **over):
    out = dict(case)
    out.update(over)
    return out


def take_image(case, img: int) -> Dict[str, object]:
    """image `img` as a call of its own: its rows, then the case's slack (what lay behind it in the batch is gone)"""
    images, npq, npk, D = case["images"], case["npad_q"], case["npad_k"], case["heads"] * HD
    rq, rk = slice(img * npq, (img + 1) * npq), slice(img * npk, (img + 1) * npk)
    vt = case["vt"][:D * images * npk].reshape(D, images, npk)[:, img].reshape(-1)
    out = _derive(case, images=1, q=np.concatenate([case["q"][rq], case["q"][-SLACK:]]), k=np.concatenate([case["k"][rk], case["k"][-SLACK:]]),
                  vt=np.concatenate([vt, case["vt"][-SLACK:]]), targets=case["targets"][img:img + 1])
    if case["bias"] is not None:
        b = case["bias"]
        out["bias"] = dict(b, qcode=np.concatenate([b["qcode"][rq], b["qcode"][-SLACK:]]), kcode=np.concatenate([b["kcode"][rk], b["kcode"][-SLACK:]]))
    return out


def take_head(case, h: int) -> Dict[str, object]:
    """head `h` as a call of one head"""
    images, npk, D = case["images"], case["npad_k"], case["heads"] * HD
    sl = slice(h * HD, (h + 1) * HD)
    vt = case["vt"][:D * images * npk].reshape(D, images * npk)[sl].reshape(-1)
    out = _derive(case, heads=1, q=np.ascontiguousarray(case["q"][:, sl]), k=np.ascontiguousarray(case["k"][:, sl]),
                  vt=np.concatenate([vt, case["vt"][-SLACK:]]), targets=case["targets"][:, h:h + 1])
    if case["bias"] is not None:
        b = case["bias"]
        out["bias"] = dict(b, w1=b["w1"][h:h + 1], wx=b["wx"][h:h + 1], wy=b["wy"][h:h + 1])
    return out


def zero_padding(case) -> Dict[str, object]:
    """the same call with zeros in every row a correct kernel reads without admitting it and may choose freely: the padding
    rows of q, k and V^T of every image and the three slacks (the case itself holds heavy values there)"""
    images, nq, n, npq, npk = (case[k] for k in ("images", "n_queries", "n_keys", "npad_q", "npad_k"))
    D = case["heads"] * HD
    q, k, vt = case["q"].copy(), case["k"].copy(), case["vt"].copy()
    q[images * npq:] = 0
    k[images * npk:] = 0
    vt[D * images * npk:] = 0
    q[:images * npq].reshape(images, npq, D)[:, nq:] = 0
    k[:images * npk].reshape(images, npk, D)[:, n:] = 0
    vt[:D * images * npk].reshape(D, images, npk)[:, :, n:] = 0
    return _derive(case, q=q, k=k, vt=vt)
