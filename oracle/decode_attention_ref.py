"""ORACLE-SIDE TEST INFRASTRUCTURE (not product code) — decode attention of the TrOCR decoder in fp64, and the operand sets the
kernel-level tests feed to ``mhip_decode_attention_host``.

One decoder step attends with one query per hypothesis (self-attention over the hypothesis' own history) or ``nq`` queries per
crop (encoder-attention over the crop's projected encoder tokens): fairseq ``MultiheadAttention`` for a single query position
with ``q`` already projected and scaled — ``softmax(K_h q_h) V_h`` per head of 64.  The self-attention history is never
re-ordered in the product (csrc/trocr_api.hip): key ``s`` of hypothesis ``r`` lives at history row ``[s][anc[r][s]]``, where
``anc`` is built step by step by ``ancestry_kernel`` (``anc_new[r][0..step] = anc_old[parent[r]][0..step]``,
``anc_new[r][step + 1] = r``; step 0 reads its own slot).  ``beam_ancestry`` replays that recurrence with random parents inside
each crop's beams, so rows of one crop share prefixes and read other rows' keys.

The operand sets are built so that the likely indexing bugs of a kernel move the result far beyond the tests' bars: each row's
queries point at one key of its history — the last, the first, or one just past a 4-, 16-, 32- or 64-key boundary — so that key
carries a large share of the softmax weight.  ``mutations`` names those bugs as changes of the reference computation; the CPU
test (tests/test_oracle_decode_attention.py) asserts that each one moves the reference by at least ten times the bar.

Only ``tests/`` may import this module.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

DISPATCH = (64, 256, 640)       # f16 short-history kernel up to 64 keys; generic (1, 256) up to 256; generic (4, 640) up to 640

# n_keys of the self-attention sweep, against the three dispatch thresholds (64, 256, 640):
#                    fast f16 kernel (<= 64)             | generic (1, 256)           | generic (4, 640)
SELF_N_KEYS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 200, 201, 255, 256, 257, 511, 640)
CROSS_N_KEYS = (1, 17, 64, 65, 256, 257, 577, 640)


def rounded(a: np.ndarray, f16: bool) -> np.ndarray:
    """the operand as the kernel sees it (fp32 array holding f16-representable values in the f16 mode)"""
    return a.astype(np.float16).astype(np.float32) if f16 else a.astype(np.float32)


def beam_ancestry(rng: np.random.Generator, crops: int, beam: int, n_keys: int, anc_ld: int) -> np.ndarray:
    """ancestry table [crops * beam][anc_ld] after n_keys - 1 steps of a beam search with random parents within the crop.  A
    row never continues itself (beam > 1), so its slot differs from one step to the next — reading step s +- 1's slot shows."""
    M = crops * beam
    anc = np.zeros((M, anc_ld), np.int32)
    anc[:, 0] = np.arange(M)
    r = np.arange(M)
    for step in range(n_keys - 1):
        hop = rng.integers(1, beam, size=M) if beam > 1 else np.zeros(M, np.int64)
        parent = (r // beam) * beam + (r % beam + hop) % beam
        new = anc.copy()                                  # columns past step + 1 keep stale (valid) slots, as in the product
        new[:, :step + 1] = anc[parent, :step + 1]
        new[:, step + 1] = np.arange(M)
        anc = new
    return anc


def target_keys(n_keys: int, rows: int) -> np.ndarray:
    """the key each row's queries point at: the last on every other row (its slot is the row's own, unshared), else the first or
    one just past a 4-, 16-, 32- or 64-key boundary"""
    cands = []
    for b in [0] + [b for b in (4, 16, 32, 64) if b < n_keys - 1]:
        cands += [n_keys - 1, b]
    return np.array([cands[r % len(cands)] for r in range(rows)], np.int64)


def self_case(seed: int, heads: int, n_keys: int, crops: int, beam: int, f16: bool) -> Dict[str, object]:
    """operands of one self-attention call: q [rows][D], k / v [n_keys][slots][D], anc [rows][anc_ld] (rows = slots)"""
    rng = np.random.default_rng(seed)
    D, M = heads * 64, crops * beam
    anc_ld = n_keys + 1 + int(rng.integers(0, 3))        # the product's pitch is max_len + 2 >= n_keys + 1
    anc = beam_ancestry(rng, crops, beam, n_keys, anc_ld)
    k = rounded(rng.normal(0, 1.0, (n_keys, M, D)), f16)
    v = rounded(rng.normal(0, 1.0, (n_keys, M, D)), f16)
    tgt = target_keys(n_keys, M)
    kt = k[tgt, anc[np.arange(M), tgt]].reshape(M, heads, 64)              # the key each row points at
    # |k_h| ~ 8: 0.75 x unit direction x 8 gives the target a score lead of ~6 over the typical key (~400 x its weight): a
    # large share of the softmax weight even among 640 keys
    unit = kt / np.linalg.norm(kt, axis=-1, keepdims=True)
    q = rounded((0.75 * unit + rng.normal(0, 0.06, (M, heads, 64))).reshape(M, D), f16)
    return {"q": q, "k": k, "v": v, "anc": anc, "heads": heads, "n_keys": n_keys, "nq": 1, "slots": M, "kv_rows": 0}


def cross_case(seed: int, heads: int, n_keys: int, groups: int, nq: int, f16: bool) -> Dict[str, object]:
    """operands of one encoder-attention call: q [groups * nq][D], k / v [groups][kv_rows][D] with NaN in the padding rows"""
    rng = np.random.default_rng(seed)
    D, rows = heads * 64, groups * nq
    kv_rows = (n_keys + 8) // 8 * 8                       # > n_keys: the product pads the 577 tokens to 584 rows
    k = np.full((groups, kv_rows, D), np.nan, np.float32)
    v = np.full((groups, kv_rows, D), np.nan, np.float32)
    k[:, :n_keys] = rounded(rng.normal(0, 1.0, (groups, n_keys, D)), f16)
    v[:, :n_keys] = rounded(rng.normal(0, 1.0, (groups, n_keys, D)), f16)
    tgt = target_keys(n_keys, rows)
    kt = k[np.arange(rows) // nq, tgt].reshape(rows, heads, 64)
    unit = kt / np.linalg.norm(kt, axis=-1, keepdims=True)
    q = rounded((0.75 * unit + rng.normal(0, 0.06, (rows, heads, 64))).reshape(rows, D), f16)
    return {"q": q, "k": k, "v": v, "anc": None, "heads": heads, "n_keys": n_keys, "nq": nq, "slots": 0, "kv_rows": kv_rows}


def attention(q: np.ndarray, K: np.ndarray, V: np.ndarray, heads: int) -> np.ndarray:
    """fp64 softmax attention: q [rows][D], K / V [rows][S][D] (the keys each row attends over) -> [rows][D]"""
    rows, S = K.shape[0], K.shape[1]
    qh = q.astype(np.float64).reshape(rows, heads, 64)
    Kh = K.astype(np.float64).reshape(rows, S, heads, 64)
    Vh = V.astype(np.float64).reshape(rows, S, heads, 64)
    s = np.einsum("rshd,rhd->rhs", Kh, qh)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    return np.einsum("rhs,rshd->rhd", p, Vh).reshape(rows, heads * 64)


def keys_of(case: Dict[str, object], anc: Optional[np.ndarray] = None, steps: Optional[np.ndarray] = None):
    """K / V [rows][S][D] each row attends over.  self: key s of row r is history row [steps[s]][anc[r][s]] (steps defaults
    to 0..n_keys-1; a mutation may pass other ancestry or drop steps); cross: the first n_keys rows of the row's group"""
    q, k, v, n = case["q"], case["k"], case["v"], case["n_keys"]
    rows = q.shape[0]
    if case["anc"] is None:
        g = np.arange(rows) // case["nq"]
        idx = np.arange(n) if steps is None else steps
        return k[g][:, idx], v[g][:, idx]
    anc = case["anc"] if anc is None else anc
    idx = np.arange(n) if steps is None else steps
    slot = anc[:, idx]                                              # [rows][S]
    return k[idx[None, :], slot], v[idx[None, :], slot]


def reference(case: Dict[str, object]) -> np.ndarray:
    K, V = keys_of(case)
    return attention(case["q"], K, V, case["heads"])


def mutations(case: Dict[str, object]) -> Dict[str, np.ndarray]:
    """the reference under each likely kernel bug that applies to the case's shape"""
    n, heads, q = case["n_keys"], case["heads"], case["q"]
    out = {}
    if n >= 2:
        K, V = keys_of(case, steps=np.arange(n - 1))
        out["drop_last_key"] = attention(q, K, V, heads)
        K, V = keys_of(case, steps=np.arange(1, n))
        out["drop_first_key"] = attention(q, K, V, heads)
    anc = case["anc"]
    if anc is not None:
        if n >= 2:
            s = np.arange(n)
            for name, src in (("anc_from_step_plus_1", np.minimum(s + 1, n - 1)), ("anc_from_step_minus_1", np.maximum(s - 1, 0))):
                bad = anc.copy()
                bad[:, :n] = anc[:, src]
                K, V = keys_of(case, anc=bad)
                out[name] = attention(q, K, V, heads)
        bad = np.repeat(anc[:1], anc.shape[0], axis=0)
        K, V = keys_of(case, anc=bad)
        out["row0_ancestry_for_all"] = attention(q, K, V, heads)
    ref = reference(case)
    sw = ref.reshape(ref.shape[0], heads, 64).copy()
    sw[:, [0, 1]] = sw[:, [1, 0]]
    out["swap_heads_0_1"] = sw.reshape(ref.shape)
    return out


def bars(f16: bool, ref: np.ndarray):
    """(max |d| bar, mean |d| bar) of the kernel tests, relative to max(1, max |ref|): about 2.5 x the worst errors measured over
    the sweep (f16 4.4e-4 / 4.5e-5, fp32 7.8e-7 / 3.1e-8; tests/test_decode_attention_gpu.py)"""
    scale = max(1.0, float(np.abs(ref).max()))
    return (1e-3 * scale, 1e-4 * scale) if f16 else (2e-6 * scale, 2e-6 * scale)


def self_params():
    """(id, self_case kwargs) of the sweep: every n_keys x heads {4, 8, 12, 16} x {f16, fp32}; rows (= slots) 9, 6, 10, 3 —
    never a multiple of 4, so the f16 kernel's last block of four rows is partial"""
    shapes = ((3, 3), (2, 3), (5, 2), (1, 3))
    out = []
    for i, n in enumerate(SELF_N_KEYS):
        for j, heads in enumerate((4, 8, 12, 16)):
            crops, beam = shapes[(i + j) % len(shapes)]
            for f16 in (True, False):
                out.append((f"{'f16' if f16 else 'f32'}-h{heads}-k{n}",
                            dict(seed=1000 * n + 10 * heads + f16, heads=heads, n_keys=n, crops=crops, beam=beam, f16=f16)))
    return out


def cross_params():
    """(id, cross_case kwargs): n_keys (577 = the encoder tokens, 640 = the limit) x nq {1, 3, 4} x heads {8, 16} x {f16, fp32}"""
    out = []
    for n in CROSS_N_KEYS:
        for nq in (1, 3, 4):
            for heads in (8, 16):
                for f16 in (True, False):
                    out.append((f"{'f16' if f16 else 'f32'}-h{heads}-nq{nq}-k{n}",
                                dict(seed=7 * n + 100 * nq + heads + f16, heads=heads, n_keys=n, groups=3, nq=nq, f16=f16)))
    return out
