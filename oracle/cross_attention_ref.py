"""ORACLE-SIDE TEST INFRASTRUCTURE (not product code) — the TrOCR decoder's encoder-attention with absorbed key / value
projections (csrc/cross_attn.hip) in fp64, stage by stage, with derived error bounds, a numpy emulation of the kernel's
arithmetic and the operand sets the kernel-level tests feed to ``mhip_cross_attention_stages_host``.

The three kernels and what each is judged against (all operands are f16-representable fp32; ``u16 = 2^-11``, ``u32 = 2^-24``):

  absorb_q    qt[r][h][:] = W_kt,h^T q_h, W_kt = f16(W_k log2 e) as ``pack_ca_kt`` makes it.  fp64 of the same operands;
              |d| <= u16 |ref| + 2^-25 + (64 + 4) u32 (|q| |W_kt|)                     (f16 store; fp32 sum of 64 products)
  cross_attn  ct[r][h][:] = softmax2_s(qt . E[s]) E over the crop's first n_keys rows, from the DEVICE's qt (f16, so exact as an
              input): the kernel alone.  |d| <= rel A + 2^-25 sum_s |E[s]| / L + u16 |ref| + 2^-25 with
                A    = sum_s p_s |E[s]| / sum_s p_s                                      (per dim)
                rel  = u16 + 2 ln2 ds + (n_keys + 8) u32 + 2^-21
                ds   = (ED + 2) u32 max_s(|qt| . |E[s]|)      fp32 accumulation of a score (ED terms, the exchange add counted
                       among them) and the subtraction of the reference, in log2 units; it moves every p_s by at most ln2 ds
                       relative, numerator and denominator apart: 2 ln2 ds (|ct| <= A)
                u16  the f16 rounding of P in the second product while the row sum adds the unrounded fp32 P
                (n_keys + 8) u32  the accumulations, rescales, the reciprocal and the final product;  2^-21  v_exp_f32
                2^-25 sum_s |E[s]| / L,  L = sum_s 2^(s_s - max) >= 1: a term of its own, by derivation —
                       P below 2^-14 is a subnormal f16 (absolute rounding 2^-25, not relative u16); the row sum in the kernel's
                       final units is >= L because its reference never exceeds the running maximum
  absorb_v    ao[r][h*64 + j] = W_v,h ct_h + b_v, from the DEVICE's ct.  |d| <= u16 |ref| + 2^-25 + (ED + 4) u32 (|ct| |W_v|^T + |b_v|)
  mean forms  the same with sqrt(K) for every accumulation length K; asserted as mean(err) <= mean(bound)
  end to end  fairseq MultiheadAttention (K = E W_k^T + b_k, V = E W_v^T + b_v, softmax(q_h . K_h) V_h) on the same rounded
              operands.  Bound = the absorb_v bound + |W_v| (the cross_attn bound) + (e^(2 ln2 Ds) - 1) sum_s p_s |V_h[s] - b_v|,
              Ds = max_s sum_d dqt_d |E[s][d]| + u32 max |s|, dqt = the absorb_q bound + (u16 + u32) (|q| |W_kt|) (the rounding of
              W_k log2 e to f16, the fp32 log2 e): the worst case of qt's rounding through the softmax — loose, it is the one
              overall check; the mean form takes root-sum-squares instead of sums over d.
Nothing is fitted to the kernel.  ``emulate`` (32-key tiles, reference set by tile 0 and moved when a tile exceeds it by 8, fp32
P into the row sum, f16 P into the product, f16 output) stays within the cross_attn bound on every case
(tests/test_oracle_cross_attention.py asserts <= 1.0).

Operands: every (row, head) has a target key — cycling through n_keys - 1, 0, 31 | 32, n_keys - 2, the first key of the last tile,
15 | 16, 63 | 64 — and a query of noise plus a push along that key's K_h, so that boundary keys carry weight; E differs between
crops, q between the beams of a crop.  The padding rows of a crop (and, where a crop has none, row 0 of the next crop) hold 1.5 x
the crop's heaviest key: a kernel that admits one key too many is far off.  ``VARIANTS`` are softmax trajectories (see
``make_case``); ``assert_trajectory`` checks on the scores themselves that each one happens.  ``mutations`` names likely kernel
bugs as changes of the reference.

Only ``tests/`` may import this module.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np

U16, U32 = 2.0 ** -11, 2.0 ** -24
LN2 = math.log(2.0)
LOG2E_F32 = np.float32(1.4426950408889634)
TK = 32                      # keys per tile
SLACK = 64                   # zero rows the host entry appends behind the last crop (CROSS_ATTN_SLACK_ROWS)
EDS = (256, 512, 768, 1024)
BEAMS = (1, 2, 3, 4)
HEADS = (1, 4, 12, 16)
VARIANTS = ("late_dominant", "rising", "tile0_max", "identical", "shift_plus", "shift_minus", "shift_zero")
T0 = 5                       # the common target key of the variants (tile 0)
S0 = 12.0                    # its score in log2 units
SHIFT = 200.0


def cross_slots(ed: int, w: int) -> int:
    """ring slots beside the score-exchange buffer in 160 KiB of LDS (cross_attn.hip, restated)"""
    return min(6, (160 * 1024 - 4 * w * 1024) // (TK * ed * 2))


def depth(ed: int, w: int = 1) -> int:
    """tiles in flight ahead of the one consumed: 5, 3, 2, 1 for ED 256, 512, 768, 1024 (the same for every beam width)"""
    return cross_slots(ed, w) - 1


def short_wave(ed: int, w: int) -> bool:
    """some waves issue one DMA instruction fewer per tile (the tile's 1 KiB instructions do not divide among 2 w waves)"""
    return (TK * ed * 2 // 1024) % (2 * w) != 0


def n_keys_classes(ed: int) -> Dict[str, int]:
    d = depth(ed)
    return {"1": 1, "31": 31, "32": 32, "33": 33, "32D": 32 * d, "32D+1": 32 * d + 1, "32(D+1)+1": 32 * (d + 1) + 1, "577": 577}


def f16(a) -> np.ndarray:
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def ntiles(n_keys: int) -> int:
    return (n_keys + TK - 1) // TK


# ---------------------------------------------------------------------------------------------------------------- operands
def target_cycle(n_keys: int) -> List[int]:
    cands = [n_keys - 1, 0, 31, 32, n_keys - 2, (ntiles(n_keys) - 1) * TK, 15, 16, 63, 64]
    out: List[int] = []
    for k in cands:
        if 0 <= k < n_keys and k not in out:
            out.append(k)
    return out


def make_case(ed: int, beam: int, heads: int, n_keys: int, crops: int, kv_extra: int = 0, variant: Optional[str] = None,
              seed: int = 0) -> Dict[str, object]:
    """operands of one call: q [M][D], E [crops][kv_rows][ed] (padding rows included), wk / wv [D][ed], bk / bv [D].

    variants (all (row, head) target key 5 with a score of exactly 12 log2 units, noise orthogonal to the push):
      tile0_max      nothing else: tile 0 holds the global maximum, the reference never moves
      late_dominant  the last key is 3 x key 5: 24 above tile 0's maximum, a rescale in the last tile
      rising         keys 37, 69, 101 are (1 + 7 i / 12) x key 5: tile maxima 12, 19, 26, 33 — no rescale at +7, one at +14, P of 2^7
      identical      every key of a crop is the crop's row 0
      shift_plus / shift_minus / shift_zero   late_dominant with column ed - 1 of E set to 1 and query component 0 of every head
                     feeding that column alone (W_k row zero but for it): all scores +200 / -200 / +0 log2 units through qt
    """
    assert variant is None or variant in VARIANTS
    rng = np.random.default_rng(seed)
    D, M = heads * 64, crops * beam
    kv_rows = (n_keys + 7) // 8 * 8 + kv_extra
    wk = f16(rng.normal(0, 2.0 / math.sqrt(ed), (D, ed)))
    wv = f16(rng.normal(0, 1.0 / math.sqrt(ed), (D, ed)))
    bk = rng.normal(0, 0.5, (D,)).astype(np.float32)
    bv = rng.normal(0, 0.3, (D,)).astype(np.float32)
    E = f16(rng.normal(0, 1.0, (crops, kv_rows, ed)))
    shift = variant in ("shift_plus", "shift_minus", "shift_zero")
    if variant is None:
        cyc = target_cycle(n_keys)
        tgt = np.array([[cyc[(r * heads + h) % len(cyc)] for h in range(heads)] for r in range(M)], np.int64)
        top = [int(tgt[c * beam, 0]) for c in range(crops)]
    else:
        assert n_keys >= 4 * TK + 1
        tgt = np.full((M, heads), T0, np.int64)
        top = [T0] * crops
        if variant == "identical":
            E[:, :n_keys] = E[:, :1]
        elif variant == "rising":
            for i in (1, 2, 3):
                E[:, TK * i + T0] = f16((1.0 + 7.0 * i / S0) * E[:, T0])
            top = [3 * TK + T0] * crops
        elif variant != "tile0_max":
            E[:, n_keys - 1] = f16(3.0 * E[:, T0])
            top = [n_keys - 1] * crops
    # rows a correct kernel never admits hold 1.5 x the crop's heaviest key: the caller's padding rows and, where the crop has
    # none, the next crop's row 0 (an ordinary key there)
    for c in range(crops):
        heavy = f16(1.5 * E[c, top[c]])
        if kv_rows > n_keys:
            E[c, n_keys:] = heavy
        elif c + 1 < crops:
            E[c + 1, 0] = heavy
    if shift:
        E[:, :, ed - 1] = 1.0
        wk[0::64, :] = 0.0
        wk[:, ed - 1] = 0.0
        wk[0::64, ed - 1] = 16.0
    # queries: noise + push along the target's K_h (without the bias, which is constant over the keys)
    E64, wk64 = E.astype(np.float64), wk.astype(np.float64)
    Kp = np.einsum("csd,jd->csj", E64[:, :n_keys], wk64).reshape(crops, n_keys, heads, 64)
    ci = (np.arange(M) // beam)[:, None]
    kt = Kp[ci, tgt, np.arange(heads)[None, :]]                       # [M][heads][64]
    if variant is None:
        # 0.12 noise scores N(0, ~2.2) nats against the keys (mean weight e^2.4 = 11 each): a push of ln(11 n) + 0.5 nats puts
        # about 0.6 of the weight on the target (9.3 at 577 keys)
        push = max(3.0, math.log(11.0 * n_keys) + 0.5)
        q = rng.normal(0, 0.12, (M, heads, 64)) + push * kt / (kt * kt).sum(-1, keepdims=True)
    else:
        noise = rng.normal(0, 0.06, (M, heads, 64))
        if shift:
            kt[..., 0] = 0.0
            noise[..., 0] = 0.0
        nn = (kt * kt).sum(-1, keepdims=True)
        noise -= (noise * kt).sum(-1, keepdims=True) / nn * kt
        q = noise + S0 * LN2 * kt / nn
        if shift:
            sign = {"shift_plus": 1.0, "shift_minus": -1.0, "shift_zero": 0.0}[variant]
            q[..., 0] = sign * SHIFT / float(f16(np.float32(16.0) * LOG2E_F32))
    q = f16(q.reshape(M, D))
    return {"ed": ed, "beam": beam, "heads": heads, "n_keys": n_keys, "crops": crops, "kv_rows": kv_rows, "variant": variant,
            "q": q, "E": E, "wk": wk, "wv": wv, "bk": bk, "bv": bv, "targets": tgt}


def e_flat(case, E=None) -> np.ndarray:
    """E as the device holds it: the crops back to back and the zero slack rows behind them"""
    E = case["E"] if E is None else E
    return np.concatenate([E.reshape(-1, case["ed"]), np.zeros((SLACK, case["ed"]), np.float32)])


# -------------------------------------------------------------------------------------------------------------- references
def absorbed_wkt(case) -> np.ndarray:
    """f16(W_k log2 e) [heads][64][ed], the product in fp32 as pack_ca_kt computes it"""
    return f16(case["wk"] * LOG2E_F32).astype(np.float64).reshape(case["heads"], 64, case["ed"])


def qt_stage(case, q=None):
    """(ref, hard bound, mean bound, magnitude) of absorb_q, each [M][heads][ed]"""
    q = case["q"] if q is None else q
    qh = q.astype(np.float64).reshape(-1, case["heads"], 64)
    wkt = absorbed_wkt(case)
    ref = np.einsum("rhj,hjd->rhd", qh, wkt)
    mag = np.einsum("rhj,hjd->rhd", np.abs(qh), np.abs(wkt))
    base = U16 * np.abs(ref) + 2.0 ** -25
    return ref, base + (64 + 4) * U32 * mag, base + math.sqrt(64 + 4) * U32 * mag, mag


def ct_stage(case, qt, keys=None, E=None):
    """softmax2 attention over E in fp64 from the absorbed queries qt [M][>= heads][ed].  keys: the rows of a crop attended
    (default 0 .. n_keys - 1; indices past kv_rows run on into the next crop / the slack rows).
    -> dict: ref, hard, mean [M][heads][ed], scores [M][heads][S], p (normalised)"""
    ed, beam, heads, n, crops, kv = (case[k] for k in ("ed", "beam", "heads", "n_keys", "crops", "kv_rows"))
    keys = np.arange(n) if keys is None else np.asarray(keys)
    flat = e_flat(case, E).astype(np.float64)
    M = crops * beam
    qt = np.asarray(qt, np.float64)[:, :heads]
    out = {k: np.empty((M, heads, ed)) for k in ("ref", "hard", "mean")}
    out["scores"] = np.empty((M, heads, len(keys)))
    out["p"] = np.empty((M, heads, len(keys)))
    for c in range(crops):
        rows = flat[c * kv + keys]
        sl = slice(c * beam, (c + 1) * beam)
        s = qt[sl] @ rows.T
        smag = (np.abs(qt[sl]) @ np.abs(rows).T).max(-1)[..., None]
        p = np.exp2(s - s.max(-1, keepdims=True))
        L = p.sum(-1, keepdims=True)
        ref = p @ rows / L
        A = p @ np.abs(rows) / L
        tail = 2.0 ** -25 * np.abs(rows).sum(0)[None, None, :] / L + U16 * np.abs(ref) + 2.0 ** -25
        S = len(keys)
        out["ref"][sl] = ref
        out["hard"][sl] = (U16 + 2 * LN2 * (ed + 2) * U32 * smag + (S + 8) * U32 + 2.0 ** -21) * A + tail
        out["mean"][sl] = (U16 + 2 * LN2 * math.sqrt(ed + 2) * U32 * smag + math.sqrt(S + 8) * U32 + 2.0 ** -21) * A + tail
        out["scores"][sl] = s
        out["p"][sl] = p / L
    return out


def ao_stage(case, ct):
    """(ref, hard, mean) [M][D] of absorb_v from the contexts ct [M][>= heads][ed]"""
    heads, ed = case["heads"], case["ed"]
    ct = np.asarray(ct, np.float64)[:, :heads]
    wv = case["wv"].astype(np.float64).reshape(heads, 64, ed)
    bv = case["bv"].astype(np.float64).reshape(1, heads, 64)
    ref = (np.einsum("rhd,hjd->rhj", ct, wv, optimize=True) + bv).reshape(ct.shape[0], -1)
    mag = (np.einsum("rhd,hjd->rhj", np.abs(ct), np.abs(wv), optimize=True) + np.abs(bv)).reshape(ct.shape[0], -1)
    base = U16 * np.abs(ref) + 2.0 ** -25
    return ref, base + (ed + 4) * U32 * mag, base + math.sqrt(ed + 4) * U32 * mag


def fairseq_reference(case, q=None, E=None, with_bk: bool = True) -> np.ndarray:
    """fairseq MultiheadAttention for one query position per row, q projected and scaled: [M][D]"""
    beam, heads, n, crops = case["beam"], case["heads"], case["n_keys"], case["crops"]
    q = (case["q"] if q is None else q).astype(np.float64).reshape(crops, beam, heads, 64)
    E = (case["E"] if E is None else E).astype(np.float64)[:, :n]
    K = np.einsum("csd,jd->csj", E, case["wk"].astype(np.float64)) + (case["bk"].astype(np.float64) if with_bk else 0.0)
    V = np.einsum("csd,jd->csj", E, case["wv"].astype(np.float64)) + case["bv"].astype(np.float64)
    s = np.einsum("cshj,cbhj->cbhs", K.reshape(crops, n, heads, 64), q)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("cbhs,cshj->cbhj", p, V.reshape(crops, n, heads, 64)).reshape(crops * beam, heads * 64)


def stages(case, qt, ct, e2e: bool = True) -> Dict[str, np.ndarray]:
    """references and bounds of the three stages from the taps qt / ct the device (or, on the CPU, a model of it) produced,
    and (e2e) of the end-to-end output"""
    ed, beam, heads, n, crops, kv = (case[k] for k in ("ed", "beam", "heads", "n_keys", "crops", "kv_rows"))
    qt = np.asarray(qt, np.float64)[:, :heads]
    out = {}
    out["qt_ref"], out["qt_hard"], out["qt_mean"], qmag = qt_stage(case)
    c = ct_stage(case, qt)
    out["ct_ref"], out["ct_hard"], out["ct_mean"] = c["ref"], c["hard"], c["mean"]
    out["ao_ref"], out["ao_hard"], out["ao_mean"] = ao_stage(case, ct)
    if not e2e:
        return out
    out["e2e_ref"] = fairseq_reference(case)
    # propagation: qt's error -> scores -> p -> the output (V without its bias: the weights sum to 1)
    wv = case["wv"].astype(np.float64).reshape(heads, 64, ed)
    flat = e_flat(case).astype(np.float64)
    M = crops * beam
    soft_h, soft_m = np.empty((M, heads, 64)), np.empty((M, heads, 64))
    for cr in range(crops):
        rows = flat[cr * kv:cr * kv + n]
        sl = slice(cr * beam, (cr + 1) * beam)
        absV = np.abs(rows @ wv.reshape(-1, ed).T).reshape(n, heads, 64)
        AV = np.einsum("bhs,shj->bhj", c["p"][sl], absV, optimize=True)
        smax = np.abs(c["scores"][sl]).max(-1)
        for hard in (True, False):
            dq = (out["qt_hard"] if hard else out["qt_mean"])[sl] + (U16 + U32) * qmag[sl]
            if hard:
                Ds = (dq @ np.abs(rows).T).max(-1) + U32 * smax
            else:
                Ds = np.sqrt((dq * dq) @ (rows * rows).T).max(-1) + U32 * smax
            (soft_h if hard else soft_m)[sl] = np.expm1(2 * LN2 * Ds)[..., None] * AV
    out["e2e_hard"] = out["ao_hard"] + (np.einsum("rhd,hjd->rhj", out["ct_hard"], np.abs(wv), optimize=True) + soft_h).reshape(M, -1)
    out["e2e_mean"] = out["ao_mean"] + (np.sqrt(np.einsum("rhd,hjd->rhj", out["ct_mean"] ** 2, wv * wv, optimize=True)) + soft_m).reshape(M, -1)
    return out


# --------------------------------------------------------------------------------------------------------------- emulation
def emulate(case, qt, rescale: str = "kernel", info: bool = False):
    """the kernel's arithmetic in numpy: fp32 scores over 32-key tiles, the reference set by tile 0 and moved (for the 16 heads of
    a beam together, as the wave votes) when a tile's maximum exceeds it by more than 8, fp32 P into the row sum, f16 P into the
    product, f16 output.  rescale: "kernel"; "no_branch" (the reference never moves); "no_scaling" (it moves, the sums are not
    scaled).  -> ct [M][heads][ed] fp32 (and with info: which tiles rescaled [M][ntiles], log2 of the largest P [M][heads][ntiles])"""
    ed, beam, heads, n, crops, kv = (case[k] for k in ("ed", "beam", "heads", "n_keys", "crops", "kv_rows"))
    flat = e_flat(case)
    qt = np.asarray(qt, np.float32)[:, :heads]
    M, nt = crops * beam, ntiles(n)
    out = np.empty((M, heads, ed), np.float32)
    rescaled = np.zeros((M, nt), bool)
    pmax = np.zeros((M, heads, nt))
    with np.errstate(all="ignore"):
        for r in range(M):
            base = (r // beam) * kv
            acc = np.zeros((heads, ed), np.float32)
            lsum = np.zeros(heads, np.float32)
            mref = np.zeros(heads, np.float32)
            for t in range(nt):
                rows = flat[base + t * TK:base + (t + 1) * TK]
                s = qt[r] @ rows.T
                s[:, max(0, n - t * TK):] = -np.inf
                mx = s.max(1)
                if t == 0:
                    mref = mx.copy()
                elif rescale != "no_branch" and bool((mx > mref + np.float32(8)).any()):
                    nr = np.maximum(mref, mx)
                    f = np.exp2(mref - nr)
                    mref = nr
                    rescaled[r, t] = True
                    if rescale != "no_scaling":
                        lsum = lsum * f
                        acc = acc * f[:, None]
                pe = np.exp2(s - mref[:, None])
                lsum = lsum + pe.sum(1, dtype=np.float32)
                acc = acc + f16(pe) @ rows
                pmax[r, :, t] = mx - mref
            out[r] = f16(acc * (np.float32(1) / lsum)[:, None])
    return (out, {"rescaled": rescaled, "log2_pmax": pmax}) if info else out


def assert_trajectory(case, qt) -> None:
    """the variant's softmax trajectory happens, judged on the scores the absorbed queries qt give"""
    v, n, heads = case["variant"], case["n_keys"], case["heads"]
    if v is None:
        return
    c = ct_stage(case, qt)
    s = c["scores"]
    nt = ntiles(n)
    tmax = np.stack([s[..., t * TK:(t + 1) * TK].max(-1) for t in range(nt)], -1)          # [M][heads][ntiles]
    _, inf = emulate(case, qt, info=True)
    if v == "identical":
        assert np.ptp(s, axis=-1).max() <= 1e-9 * max(1.0, np.abs(s).max()), "identical keys, identical scores"
        want = np.repeat(case["E"][:, 0].astype(np.float64), case["beam"], axis=0)[:, None, :]
        assert np.abs(c["ref"] - want).max() <= 1e-12
        return
    if v == "tile0_max":
        assert (tmax[..., 0:1] >= tmax).all() and not inf["rescaled"].any()
        return
    if v == "rising":
        step = np.diff(tmax[..., :4], axis=-1)
        assert (np.abs(step - 7.0) <= 0.5).all(), "tile maxima rise by about 7 log2 units over the first four tiles"
        assert not inf["rescaled"][:, 1].any() and inf["rescaled"][:, 2].all() and not inf["rescaled"][:, 3].any()
        assert (inf["log2_pmax"][..., 1] >= 6.5).all() and (inf["log2_pmax"][..., 3] >= 6.5).all() and inf["log2_pmax"].max() <= 8.0
        assert (tmax[..., 3] - tmax[..., 0] >= 20.0).all()
        return
    # late_dominant and the shifts: the last tile outgrows everything before it by more than 16 (a rescale at t = ntiles - 1 > 0;
    # without it P would leave the f16 range)
    lead = tmax[..., -1] - tmax[..., :-1].max(-1)
    assert (lead >= 20.0).all() and inf["rescaled"][:, -1].all() and not inf["rescaled"][:, :-1].any()
    if v in ("shift_plus", "shift_minus"):
        sign = 1.0 if v == "shift_plus" else -1.0
        assert (sign * s[..., :n - 1] >= SHIFT - 16.0).all() and (sign * s[..., :n - 1] <= SHIFT + 16.0).all()


# --------------------------------------------------------------------------------------------------------------- mutations
def mutations(case, qt, ct=None) -> Dict[str, Tuple[str, np.ndarray]]:
    """name -> (stage, result under that kernel bug), for the bugs that apply to the case.  stage "ct": compare with the cross_attn
    reference from the same qt; "ao": with the absorb_v reference from the same ct.  Dropping a key applies where some (row, head)
    targets it."""
    n, heads, beam, crops, kv = case["n_keys"], case["heads"], case["beam"], case["crops"], case["kv_rows"]
    v = case["variant"]
    # keys that carry weight: the targets; in the variants only the dominant last key of late_dominant and the shifts
    tg = set(case["targets"].ravel().tolist()) if v is None else ({n - 1} if v == "late_dominant" or v.startswith("shift") else set())
    out: Dict[str, Tuple[str, np.ndarray]] = {}
    keys = np.arange(n)
    if n >= 2:
        for name, k in (("drop_last_key", n - 1), ("drop_first_key", 0), ("drop_key_31", 31), ("drop_key_32", 32)):
            if k in tg:
                out[name] = ("ct", ct_stage(case, qt, keys=keys[keys != k])["ref"])
    if kv > n or crops > 1:          # the admitted row is the caller's: padding or the next crop's first row
        out["admit_key_n"] = ("ct", ct_stage(case, qt, keys=np.arange(n + 1))["ref"])
    if heads >= 2 and ct is not None:      # absorb_v writing head 0's block where head 1's belongs
        sw = ao_stage(case, ct)[0].reshape(-1, heads, 64).copy()
        sw[:, [0, 1]] = sw[:, [1, 0]]
        out["swap_heads_0_1"] = ("ao", sw.reshape(sw.shape[0], -1))
    # cross_attn reading another beam's queries / another crop's tokens: judged on the contexts (tighter than end to end).  With one
    # key, or in the variants (every beam's weight on the same keys), the contexts do not depend on the query: not a visible bug
    if beam >= 2 and n >= 2 and v is None:
        q0 = np.asarray(qt)[:, :heads].reshape(crops, beam, heads, -1)[:, :1].repeat(beam, axis=1).reshape(crops * beam, heads, -1)
        out["beam0_queries_for_all"] = ("ct", ct_stage(case, q0)["ref"])
    if crops >= 2:
        out["crop0_E_for_all"] = ("ct", ct_stage(case, qt, E=np.repeat(case["E"][:1], crops, axis=0))["ref"])
    if case["variant"] in ("late_dominant", "rising", "shift_plus", "shift_minus", "shift_zero"):
        out["no_rescale_branch"] = ("ct", emulate(case, qt, rescale="no_branch").astype(np.float64))
        out["rescale_without_scaling"] = ("ct", emulate(case, qt, rescale="no_scaling").astype(np.float64))
    return out


def moved(mut: np.ndarray, ref: np.ndarray, bound: np.ndarray) -> float:
    """the largest |mut - ref| / bound over the elements; a non-finite result counts as infinitely far"""
    if not np.isfinite(mut).all():
        return math.inf
    return float((np.abs(mut - ref) / bound).max())


# -------------------------------------------------------------------------------------------------------------- case tables
def _kw(ed, beam, heads, n, crops, extra, variant=None):
    vid = f"-{variant}" if variant else ""
    vi = 0 if variant is None else 1 + VARIANTS.index("shift_plus" if variant.startswith("shift") else variant)   # the shifts share operands
    seed = ed * 7 + beam * 1009 + heads * 31 + n * 13 + crops * 3 + extra + vi * 100003
    return (f"ed{ed}-w{beam}-h{heads}-k{n}-c{crops}-x{extra}{vid}",
            dict(ed=ed, beam=beam, heads=heads, n_keys=n, crops=crops, kv_extra=extra, variant=variant, seed=seed))


def variant_n_keys(ed: int) -> int:
    """at least five tiles (the rising trajectory needs four and a last tile) and more tiles than the ring is deep"""
    return max(4 * TK + 1, 32 * (depth(ed) + 1) + 1)


def sweep_params():
    """every ED x beam x n_keys class; heads 1 / 4 / 12 / 16, crops 1 .. 3 and kv_rows npad / npad + 8 rotated through the table"""
    out = []
    for ei, ed in enumerate(EDS):
        seen = set()
        for ki, n in enumerate(n_keys_classes(ed).values()):
            if n in seen:
                continue
            seen.add(n)
            for beam in BEAMS:
                heads = HEADS[(ki + beam + ei) % 4]
                crops = 1 + (ki + beam) % 3
                extra = 8 * ((ki + beam + ei) % 2)
                if crops == 1 and extra == 0 and n % 8 == 0:
                    crops = 2               # no padding rows: the row behind the last key is the next crop's
                out.append(_kw(ed, beam, heads, n, crops, extra))
    return out


def rows68_params():
    """17 crops x beam 4 = 68 query rows: a full 64-row block of the absorb kernels and a partial one"""
    return [_kw(ed, 4, HEADS[(i + 1) % 4], 32 * depth(ed) + 1, 17, 8 * (i % 2)) for i, ed in enumerate(EDS)]


def variant_params():
    """each trajectory on one shape per ED: beam 3 (short waves at ED 256, 512, 1024), 2 crops"""
    return [_kw(ed, 3, HEADS[(i + 1) % 4] if HEADS[(i + 1) % 4] > 1 else 16, variant_n_keys(ed), 2, 8 * (i % 2), v)
            for i, ed in enumerate(EDS) for v in VARIANTS]


def all_params():
    return sweep_params() + rows68_params() + variant_params()


def isolation_params():
    """a few shapes per ED for the bit-for-bit isolation checks: W = 3 with 577 keys, and a ring edge with padding / without"""
    out = []
    for i, ed in enumerate(EDS):
        d = depth(ed)
        out += [_kw(ed, 3, HEADS[(i + 2) % 4] if HEADS[(i + 2) % 4] > 1 else 12, 577, 3, 8),
                _kw(ed, 4, 16, 32 * d + 1, 2, 0),
                _kw(ed, 2, 4, 32 * (d + 1), 3, 0)]
    return out
