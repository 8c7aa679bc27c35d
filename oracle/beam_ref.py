"""ORACLE (test infrastructure, not product code) — the TrOCR decoder's per-step beam search restated in numpy, for the kernel-level
tests of ``mhip_beam_candidates_host`` and ``mhip_beam_search_host`` (csrc/trocr_ops.hip: beam_candidates_kernel, ancestry_kernel;
csrc/beam_state.hip: beam_init / beam_select / beam_best).  No torch, no product imports.

    candidates      log_softmax + masks + cumulative score + stable descending order, in fp64 on the logits as the device holds them
    select / ancestry / best / init_state / search
                    integer-exact restatements of oracle/trocr_torch.py:176-213 and of the ancestry recurrence, with the device's
                    double buffering of the token and ancestry tables
    score_bound     the per-candidate bound on |score_dev - score_ref| (derivation in its docstring)
    emulate_candidates
                    the kernel's arithmetic in fp32 numpy — chunking, running maximum, merge order, 64-bit keys and the three
                    selection stages — optionally with one of CAND_MUTATIONS seeded
    GPU_CASES / case_params / make_case, SEARCH_SHAPES / make_search, list_cases
                    the seeded cases of tests/test_beam_gpu.py; tests/test_oracle_beam.py proves on the CPU that they decide

What the device leaves unspecified is marked here: after a crop has finished, its rows of the token buffer, ``cum`` and ``ignore``
are whatever they were (the reference holds UNSPEC / NaN / 255 there) and ``live_rows`` names the rows a test compares.
One thing is the device's own where the generator has no defined result: a crop that reaches step max_len is finished whether or
not anything was finalised (the generator would index an empty list); ``best`` then returns length 0, -inf and a row of pad.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24                 # unit roundoff of fp32
L2E = np.float32(1.4426950408889634)
THREADS, WAVES, CAND_K = 1024, 16, 8
GUARD = 16                       # guard elements behind each list of mhip_beam_candidates_host
UNSPEC = -2                      # token cells of a finished crop
NINF = -np.inf


def epc(f16: bool) -> int:
    """elements of one 16-byte chunk"""
    return 8 if f16 else 4


# ---------------------------------------------------------------------------------------------------------------- candidates
def _row_lse(x):
    """fp64 logsumexp of one row as log_softmax defines it: NaN for a row with a NaN, a +inf or nothing but -inf"""
    with np.errstate(all="ignore"):
        mx = np.max(x)                    # NaN propagates
        return mx + np.log(np.sum(np.exp(x - mx)))


def candidates(logits, cum, step, max_len, min_len, pad, eos, vocab, beam, bsz):
    """logits [bsz*beam][ld] in the device's type, cum [bsz*beam].  Per crop: "scores" fp64 [nb * vocab] over the flat index
    b * vocab + token (nb = 1 at step 0), "order" the stable descending order, and the first 2 * beam of it as
    "cand_scores" / "cand_tokens" / "cand_beams"; "bound" [nb * vocab] is score_bound of every entry."""
    K2 = 2 * beam
    nb = 1 if step == 0 else beam
    x = np.asarray(logits)[:, :vocab].astype(np.float64).reshape(bsz, beam, vocab)
    cum = np.asarray(cum, np.float64).reshape(bsz, beam)
    out = []
    for s in range(bsz):
        sc = np.empty((nb, vocab))
        bd = np.empty((nb, vocab))
        for b in range(nb):
            with np.errstate(all="ignore"):
                lp = x[s, b] - _row_lse(x[s, b])
            lp[lp != lp] = NINF
            if 0 <= pad < vocab:
                lp[pad] = NINF
            if step >= max_len:
                keep = lp[eos]
                lp[:] = NINF
                lp[eos] = keep
            elif step < min_len:
                lp[eos] = NINF
            sc[b] = lp if step == 0 else lp + cum[s, b]
            bd[b] = score_bound(x[s, b], 0.0 if step == 0 else cum[s, b], np.asarray(logits).dtype == np.float16)
            bd[b][sc[b] == NINF] = 0.0
        flat = sc.reshape(-1)
        order = np.argsort(-flat, kind="stable")
        top = order[:K2]
        out.append({"scores": flat, "bound": bd.reshape(-1), "order": order, "cand_scores": flat[top],
                    "cand_tokens": (top % vocab).astype(np.int32), "cand_beams": (top // vocab).astype(np.int32)})
    return out


def score_bound(row, cum, f16):
    """Bound on |score_dev - score_ref| of every element of one row (fp64 logits ``row`` [vocab], the row's cumulative score).

    The kernel computes, all in fp32 (u = u32 = 2^-24), with m the running maximum and mx the row's maximum:
        t = (f - m) * L2E; sum += exp2(t)          per element; per thread one rescale sum *= exp2((m - cm) * L2E) per chunk
        (m, sum) pairs merged over 6 shuffle rounds, then 16 wave partials     each merge: one exp2, one multiply, one addition
        lse = mx + logf(ss);  lp = f - lse;  score = lp + cum
    * The argument of every exp2: the subtraction and the product round (2 u) and L2E is the fp32 nearest to log2(e) (u), so an
      element that sits d = mx - f below the maximum carries a relative error 3 u d in its term, however the distance d is split
      over rescales (m only grows, the pieces add up to d).  Weighted by the element's share p_i of the sum: 3 u sum_i p_i d_i,
      computed here in fp64 from the row itself.
    * SUPPOSED, not measured: the hardware exp2 (v_exp_f32) and logf are each taken as accurate to 1 ulp = 2 u relative.  A term
      passes through at most `stages` = chunks per thread + 6 + 1 rescales, each an exp2 (2 u) and a product (u), after its own
      exp2 (2 u): (3 stages + 2) u.
    * Additions: all terms are positive, so a chain of L additions costs L u relative; the longest chain is EPC * chunks per
      thread + 6 + 16.
    * Terms below 2^-126 are flushed: vocab * 2^-126 absolute on a sum that is at least 1.
    * logf(ss): its relative error 2 u on |log ss|, plus the relative error of ss itself (d log = d ss / ss).
    * The three roundings of mx + logf(ss), f - lse and lp + cum: u (|lse| + |lp| + |score|) — and, since fl(a + b) is never further
      from a + b than the smaller operand is from 0, each of them at most its smaller operand: |logf(ss)|, |f| and |cum|.  That is
      what makes a row with one logit of 1e30 decidable: ss = 1, logf(ss) = 0, lse = mx exactly, the winner's score is cum exactly,
      where u |lse| = 6e22 would bound nothing.
    First order in u throughout; the measured max err / bound of tests/test_beam_gpu.py shows whether the supposed ulps held."""
    row = np.asarray(row, np.float64)
    V = row.shape[0]
    e = epc(f16)
    nct = -(-(-(-V // e)) // THREADS)                     # chunks per thread, rounded up
    with np.errstate(all="ignore"):
        mx = np.max(row)
        d = mx - row
        w = np.exp(-d)
        ss = np.sum(w)
        pd = np.where(w > 0, w * d, 0.0).sum() / ss
        lse = mx + np.log(ss)
        lp = row - lse
        sc = lp + cum
        stages = nct + 6 + 1
        chain = e * nct + 6 + 16
        rel_ss = U32 * (3 * pd + 3 * stages + 2 + chain) + V * 2.0 ** -126
        log_err = rel_ss + 2 * U32 * abs(np.log(ss))
        r_lse = min(U32 * abs(lse), abs(np.log(ss)) + log_err)
        r_lp = np.minimum(U32 * np.abs(lp), np.abs(row))
        r_sc = np.minimum(U32 * np.abs(sc), abs(cum))
        b = log_err + r_lse + r_lp + r_sc
    return np.where(np.isfinite(b), b, 0.0)               # a row that is -inf everywhere has no finite score to bound


def tie_is_exact(case, s, fa, fb):
    """two flat entries of crop s that the reference scores equal: does the device see equal bits too?  Both -inf; or equal logits
    in rows that hold the same bits with the same cum (one row, or identical rows)."""
    vocab, beam = case["vocab"], case["beam"]
    ref = case["_ref"][s]["scores"]
    if ref[fa] == NINF and ref[fb] == NINF:
        return True
    L = case["logits"]
    ra, rb = s * beam + fa // vocab, s * beam + fb // vocab
    same_rows = ra == rb or (L[ra, :vocab].tobytes() == L[rb, :vocab].tobytes() and case["cum"][ra] == case["cum"][rb])
    return bool(same_rows and L[ra, fa % vocab] == L[rb, fb % vocab])


# ------------------------------------------------------------------------------------------ the kernel's arithmetic, emulated
CAND_MUTATIONS = ("tie_high_index", "shortlist_k_minus_1", "drop_wave_partial", "padding_in_max", "pad_unmasked",
                  "beam_rows_at_step0", "cum_at_step0", "inf_chunk_nan", "min_len_if", "nan_chunk_skipped")


LSE_MUTATIONS = ("drop_wave_partial", "padding_in_max", "inf_chunk_nan", "nan_chunk_skipped")


def _exp2(t):
    with np.errstate(all="ignore"):
        return np.exp2(t.astype(np.float32)).astype(np.float32)


def _emulated_lse(rowfull, vocab, e, mut):
    """one row's m + logf(ss) as the workgroup computes it.  rowfull: the row with its padding columns, fp32"""
    nch = -(-vocab // e)
    nct = -(-nch // THREADS)
    f = np.full(nct * THREADS * e, NINF, np.float32)
    n = min(len(rowfull), nch * e)
    f[:n] = rowfull[:n]
    if mut != "padding_in_max":
        f[vocab:] = NINF
    f = f.reshape(nct, THREADS, e)
    m = np.full(THREADS, NINF, np.float32)
    sm = np.zeros(THREADS, np.float32)
    with np.errstate(all="ignore"):
        for k in range(nct):
            fk = f[k]
            cm = np.fmax.reduce(fk, axis=1)                      # fmaxf: a NaN operand is ignored
            dead = cm == NINF
            nan_only = dead & np.isnan(fk).any(axis=1)
            if mut == "nan_chunk_skipped":
                nan_only[:] = False
            if mut == "inf_chunk_nan":
                dead = np.zeros_like(dead)
            run = ~dead
            up = run & (cm > m)
            sm = np.where(up, sm * _exp2((m - cm) * L2E), sm).astype(np.float32)
            m = np.where(up, cm, m)
            for j in range(e):
                sm = np.where(run, sm + _exp2((fk[:, j] - m) * L2E), sm).astype(np.float32)
            m = np.where(nan_only, np.float32(np.inf), m)       # a NaN among -inf: the row's log-sum-exp is NaN
            sm = np.where(nan_only, np.float32(np.nan), sm)
        idx = np.arange(THREADS)
        for o in (32, 16, 8, 4, 2, 1):
            om, os_ = m[idx ^ o], sm[idx ^ o]
            nm = np.fmax(m, om)
            a = np.where(m == NINF, np.float32(0), sm * _exp2((m - nm) * L2E))
            b = np.where(om == NINF, np.float32(0), os_ * _exp2((om - nm) * L2E))
            sm, m = (a + b).astype(np.float32), nm
        wm, ws = m[::64], sm[::64]
        mm = np.fmax.reduce(wm)
        ss = np.float32(0)
        for w in range(WAVES):
            if mut == "drop_wave_partial" and w == 5:
                continue
            ss = np.float32(ss + (np.float32(0) if wm[w] == NINF else np.float32(ws[w] * _exp2((wm[w] - mm) * L2E))))
        return np.float32(mm + np.log(ss, dtype=np.float32))


def _okey(sc):
    u = sc.astype(np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)


def _okey_inv(k):
    k = k.astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _neg_sort(keys):
    return np.sort(keys, axis=1)[:, ::-1]


def emulate_candidates(case, mut=None):
    """-> (cand_scores fp32, cand_tokens, cand_beams), each [bsz][2 * beam], as beam_candidates_kernel computes them"""
    vocab, beam, bsz, step = case["vocab"], case["beam"], case["bsz"], case["step"]
    pad, eos, max_len, min_len = case["pad"], case["eos"], case["max_len"], case["min_len"]
    e = epc(case["f16"])
    K = 2 * beam
    short = K - 1 if mut == "shortlist_k_minus_1" else K
    nb = beam if (step > 0 or mut == "beam_rows_at_step0") else 1
    L = case["logits"].astype(np.float32)
    nch = -(-vocab // e)
    nct = -(-nch // THREADS)
    cs = np.empty((bsz, K), np.float32)
    ct = np.empty((bsz, K), np.int32)
    cb = np.empty((bsz, K), np.int32)
    for s in range(bsz):
        keys = np.zeros((nb, nct * THREADS * e), np.uint64)
        for b in range(nb):
            row = L[s * beam + b]
            lkey = (s * beam + b, mut if mut in LSE_MUTATIONS else None)       # the other bugs leave the log-sum-exp alone
            if lkey not in case.setdefault("_lse", {}):
                case["_lse"][lkey] = _emulated_lse(row, vocab, e, mut)
            lse = case["_lse"][lkey]
            base = np.float32(case["cum"][s * beam + b]) if (step > 0 or mut == "cum_at_step0") else np.float32(0)
            with np.errstate(all="ignore"):
                lp = (row[:vocab] - lse).astype(np.float32)
                lp[lp != lp] = NINF
                if 0 <= pad < vocab and mut != "pad_unmasked":
                    lp[pad] = NINF
                if step >= max_len:
                    keep = lp[eos]
                    lp[:] = NINF
                    lp[eos] = keep
                # Here the clean emulation states the reference's elif, NOT the kernel: beam_candidates_kernel applies the two masks as
                # independent ifs, which is the "min_len_if" mutation itself.  The two differ only where min_len > max_len; both test
                # entries and mhip_trocr_create refuse that, so on the device the difference is unreachable and the refusals guard it.
                if step < min_len and (mut == "min_len_if" or step < max_len):
                    lp[eos] = NINF
                sc = (lp + base).astype(np.float32)
            flat = (b * vocab + np.arange(vocab)).astype(np.uint64)
            low = flat if mut == "tie_high_index" else np.uint64(0xFFFFFFFF) - flat
            keys[b, :vocab] = (_okey(sc) << np.uint64(32)) | low
        # thread tid owns chunks tid, tid + 1024, ... of every row: its shortlist, then its wave's, then wave 0 over the 16 lists
        per_thread = keys.reshape(nb, nct, THREADS, e).transpose(2, 0, 1, 3).reshape(THREADS, -1)
        lane = np.zeros((THREADS, K), np.uint64)
        own = _neg_sort(per_thread)[:, :short]
        lane[:, :own.shape[1]] = own
        wave = _neg_sort(lane.reshape(WAVES, 64 * K))[:, :K]
        top = _neg_sort(wave.reshape(1, -1))[0, :K]
        fl = (top & np.uint64(0xFFFFFFFF)) if mut == "tie_high_index" else np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))
        cs[s] = _okey_inv(top >> np.uint64(32))
        ct[s] = (fl % np.uint64(vocab)).astype(np.int32)
        cb[s] = (fl // np.uint64(vocab)).astype(np.int32)
    return cs, ct, cb


# --------------------------------------------------------------------------------------------------- select, ancestry, best
STATE_MUTATIONS = ("fin_score_not_divided", "finalise_past_beam", "ignored_eos_finalised", "best_last_on_tie",
                   "ancestry_own_history", "finished_parents_kept")


def init_state(bsz, beam, max_len, pad, eos, dtype=np.float32):
    M, ld = bsz * beam, max_len + 2
    tok = np.full((M, ld), pad, np.int32)
    tok[:, 0] = eos
    anc0 = np.zeros((M, ld), np.int32)
    anc0[:, 0] = np.arange(M)
    return {"bsz": bsz, "beam": beam, "max_len": max_len, "pad": pad, "eos": eos, "dtype": dtype,
            "tokens": tok, "tokens_prev": tok.copy(), "last_tok": np.full(M, eos, np.int32), "parent": np.arange(M, dtype=np.int32),
            "cum": np.zeros(M, dtype), "ignore": np.zeros(M, np.uint8), "finished": np.zeros(bsz, np.uint8),
            "fin_count": np.zeros(bsz, np.int32), "fin_tokens": np.full((bsz, beam, max_len + 1), -1, np.int32),
            "fin_len": np.full(M, -1, np.int32), "remaining": bsz,
            # never-written cells as the device's 0xff fill reads
            "fin_score": np.full(M, 0xFFFFFFFF, np.uint32).view(np.float32) if dtype == np.float32 else np.full(M, np.nan, dtype),
            "anc": anc0, "anc_other": np.full((M, ld), -1, np.int32)}


def ancestry(st, step, mut=None):
    """the table decode step `step` (>= 1) reads: columns 0 .. step - 1 of the parent's row, column `step` the row itself; written
    into the other buffer, whose remaining columns keep their initial fill"""
    M = st["anc"].shape[0]
    new = st["anc_other"]
    src = np.arange(M) if mut == "ancestry_own_history" else st["parent"]
    new[:, :step] = st["anc"][src, :step]
    new[:, step] = np.arange(M)
    st["anc"], st["anc_other"] = new, st["anc"]


def select(st, cs, ct, cb, step, mut=None):
    """one step of the generator's bookkeeping on the candidate lists [bsz][2 * beam] (oracle/trocr_torch.py:176-206)"""
    bsz, beam, ML, eos, dt = st["bsz"], st["beam"], st["max_len"], st["eos"], st["dtype"]
    K2 = 2 * beam
    told = st["tokens"]
    tnew = st["tokens_prev"]                                   # the other buffer: rows of live crops are rewritten below
    for s in range(bsz):
        rows = np.arange(s * beam, (s + 1) * beam)
        if st["finished"][s]:
            if mut != "finished_parents_kept":
                st["parent"][rows] = rows
                st["last_tok"][rows] = eos
            tnew[rows] = UNSPEC
            continue
        eos_mask = (ct[s] == eos) & (cs[s] != NINF)
        ign = st["ignore"][rows].astype(bool)
        if mut != "ignored_eos_finalised":
            eos_mask[:beam][ign] = False
        nfin = int(st["fin_count"][s])
        for j in range(beam):
            if eos_mask[j] and (nfin < beam or mut == "finalise_past_beam"):
                slot = min(nfin, beam - 1)
                src = s * beam + int(cb[s, j])
                st["fin_tokens"][s, slot, :step] = told[src, 1:step + 1]
                st["fin_tokens"][s, slot, step] = eos
                st["fin_len"][s * beam + slot] = step + 1
                st["fin_score"][s * beam + slot] = dt(cs[s, j]) if mut == "fin_score_not_divided" else dt(cs[s, j]) / dt(step + 1)
                nfin = min(nfin + 1, beam)
        st["fin_count"][s] = nfin
        if mut == "ignored_eos_finalised":
            eos_mask[:beam][ign] = False
        if nfin == beam or step == ML:
            st["finished"][s] = 1
            st["remaining"] -= 1
            if mut != "finished_parents_kept":
                st["parent"][rows] = rows
                st["last_tok"][rows] = eos
            tnew[rows] = UNSPEC
            st["cum"][rows] = np.nan
            st["ignore"][rows] = 255
            continue
        eos_mask[:beam] |= ign
        active = eos_mask.astype(np.int64) * K2 + np.arange(K2)
        hyp = np.argsort(active, kind="stable")[:beam]
        new_ign = active[hyp] >= K2
        newp, newl, newc = st["parent"].copy(), st["last_tok"].copy(), st["cum"].copy()
        for b in range(beam):
            j, row = int(hyp[b]), s * beam + b
            src = s * beam + int(cb[s, j])
            tnew[row] = st["pad"]
            tnew[row, :step + 1] = told[src, :step + 1]
            tnew[row, step + 1] = ct[s, j]
            newp[row], newl[row], newc[row] = src, ct[s, j], dt(cs[s, j])
        st["parent"], st["last_tok"], st["cum"] = newp, newl, newc
        st["ignore"][rows] = new_ign
    st["tokens"], st["tokens_prev"] = tnew, told


def best(st, mut=None):
    """-> tokens [bsz][max_len + 1], lengths [bsz], scores [bsz]: the highest normalised score, the first finalised on a tie"""
    bsz, beam, ML = st["bsz"], st["beam"], st["max_len"]
    tok = np.full((bsz, ML + 1), st["pad"], np.int32)
    ln = np.zeros(bsz, np.int32)
    sc = np.full(bsz, NINF, st["dtype"])
    for s in range(bsz):
        b = -1
        for j in range(int(st["fin_count"][s])):
            v = st["fin_score"][s * beam + j]
            if b < 0 or v > st["fin_score"][s * beam + b] or (mut == "best_last_on_tie" and v == st["fin_score"][s * beam + b]):
                b = j
        if b < 0:
            continue
        ln[s] = st["fin_len"][s * beam + b]
        tok[s, :ln[s]] = st["fin_tokens"][s, b, :ln[s]]
        sc[s] = st["fin_score"][s * beam + b]
    return tok, ln, sc


PER_STEP = ("cand_scores", "cand_tokens", "cand_beams", "parent", "last_tok", "cum", "ignore", "finished", "fin_count", "tokens",
            "anc", "remaining")


def search(p, lists=None, logits=None, extra_steps=0, steps=None, mut=None, dtype=np.float32):
    """The launch sequence of trocr_decode without the decoder: init; per step ancestry (step > 0), candidates, select; best.
    lists = (scores, tokens, beams) [S][bsz][2 * beam]: candidates mode (``steps``: run exactly that many, as a device run did).
    logits [S][bsz*beam][ld]: the free-running reference, ``candidates`` on its own cum (dtype fp64: nothing rounded).
    -> the trace mhip_beam_search_host copies out, as a dict of arrays [steps][...] plus the final ones."""
    bsz, beam, ML = p["bsz"], p["beam"], p["max_len"]
    st = init_state(bsz, beam, ML, p["pad"], p["eos"], dtype)
    tr = {k: [] for k in PER_STEP}
    extra, step = extra_steps, 0
    while step <= ML:
        if steps is not None:
            if step >= steps:
                break
        elif st["remaining"] == 0:
            if extra <= 0:
                break
            extra -= 1
        if step > 0:
            ancestry(st, step, mut)
        if lists is not None:
            cs, ct, cb = (np.asarray(a[step]) for a in lists)
        else:
            ref = candidates(logits[step], st["cum"], step, ML, p["min_len"], p["pad"], p["eos"], p["vocab"], beam, bsz)
            cs = np.stack([r["cand_scores"] for r in ref])
            ct = np.stack([r["cand_tokens"] for r in ref])
            cb = np.stack([r["cand_beams"] for r in ref])
        select(st, cs, ct, cb, step, mut)
        for k, v in (("cand_scores", cs), ("cand_tokens", ct), ("cand_beams", cb)):
            tr[k].append(np.array(v))
        for k in PER_STEP[3:]:
            tr[k].append(np.array(st[k]))
        step += 1
    out = {k: np.stack(v) for k, v in tr.items()}
    out["steps"] = step
    out["fin_tokens"], out["fin_len"], out["fin_score"] = st["fin_tokens"], st["fin_len"], st["fin_score"]
    out["out_tokens"], out["out_len"], out["out_score"] = best(st, mut)
    return out


def live_rows(trace, step, beam):
    """rows whose token buffer, cum and ignore are specified after `step`: those of crops not finished by then"""
    return np.repeat(trace["finished"][step] == 0, beam)


def compared(trace, beam):
    """everything a test compares of a search, unspecified cells blanked: a dict of arrays, equal bits <=> equal search"""
    out = {}
    for k in ("parent", "last_tok", "finished", "fin_count", "anc", "remaining", "fin_tokens", "fin_len", "out_tokens", "out_len"):
        out[k] = np.array(trace[k])
    for k in ("fin_score", "out_score"):
        out[k] = np.array(trace[k], np.float32).view(np.uint32)
    tok = np.array(trace["tokens"])
    cum = np.array(trace["cum"], np.float32).view(np.uint32).copy()
    ign = np.array(trace["ignore"]).copy()
    for s in range(trace["steps"]):
        dead = ~live_rows(trace, s, beam)
        tok[s, dead] = UNSPEC
        cum[s, dead] = 0
        ign[s, dead] = 255
    out["tokens"], out["cum"], out["ignore"], out["steps"] = tok, cum, ign, np.array(trace["steps"])
    return out


def differing(a, b):
    """names of the compared arrays in which two searches differ"""
    return [k for k in a if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------------- cases: the kernel alone
WIN_TOP, WIN_STEP = 9.0, 0.3125      # scripted winners: 9, 8.6875, ... (exact in f16), 4 * beam + 3 of them, dealt over the rows
SPARE = 3
PADFILL = (np.inf, np.nan, 65504.0)


def _c(vocab, beam, bsz, place="spread", seed=0, **kw):
    d = dict(vocab=vocab, beam=beam, bsz=bsz, place=place, seed=seed, step=1, max_len=6, min_len=1, pad=1, eos=2, special=None)
    d.update(kw)
    return d


def _cases():
    c = []
    for beam in (1, 2, 3, 4):
        bsz = 1 if beam % 2 else 3
        for vocab in sorted({2 * beam, 8, 9, 17, 4095, 4096, 4097, 8191, 8192, 8193}):
            c.append(_c(vocab, beam, bsz, seed=200 + beam))
        # where the winners sit decides which selection stage has to be right (vocab 8193: every thread a chunk, thread 0 two)
        for place in ("one_chunk", "one_wave", "per_wave", "col0", "last_col", "same_col") + (("rows_gt0",) if beam > 1 else ()):
            c.append(_c(8193, beam, 4 - bsz, place, seed=10 + beam))
        c.append(_c(17, beam, bsz, "constant_row", seed=20 + beam))
        c.append(_c(4097, beam, bsz, "identical_rows", seed=30 + beam))
        c.append(_c(24, beam, bsz, seed=40 + beam, step=6))                                   # step == max_len
        c.append(_c(24, beam, bsz, seed=50 + beam, step=7))                                   # step > max_len
        c.append(_c(24, beam, bsz, "on_eos", seed=60 + beam, step=2, min_len=3))              # step < min_len
        for pad in (0, 1, 16):
            c.append(_c(17, beam, bsz, "on_pad", seed=70 + beam + pad, pad=pad))
        c.append(_c(4097, beam, 3, seed=80 + beam, step=0, special="step0_nan"))
        c.append(_c(4097, beam, 3, seed=85 + beam, step=0, special="step0_decoys"))
        for special in ("nan", "nan_alone", "posinf", "neginf_row", "neginf_runs", "cum_neginf", "magnitude"):
            c.append(_c(17 if special == "nan_alone" else 8193, beam, bsz, seed=190 + beam, special=special))
    for beam in (3, 4):
        c.append(_c(50265, beam, 2, seed=100 + beam))
    return c


def case_id(kw):
    tag = f"v{kw['vocab']}-beam{kw['beam']}-bsz{kw['bsz']}-{kw['place']}-step{kw['step']}"
    if kw["special"]:
        tag += "-" + kw["special"]
    if kw["pad"] != 1:
        tag += f"-pad{kw['pad']}"
    return tag


GPU_CASES = _cases()
# the mask order shows only where min_len > max_len, which both entries refuse (and mhip_trocr_create): a CPU-only case
CPU_ONLY_CASES = [_c(24, 2, 1, seed=7, step=6, max_len=6, min_len=9)]


def case_params():
    return [(case_id(kw), kw) for kw in GPU_CASES]


def make_case(f16, vocab, beam, bsz, place, seed, step, max_len, min_len, pad, eos, special):
    """-> dict with "logits" [bsz*beam][ld] in the device's type (padding columns filled with +inf, NaN and 65504 in turn), "cum"
    fp32 [bsz*beam] and the scalars of one mhip_beam_candidates_host call"""
    rng = np.random.default_rng(1000 * seed + (1 if f16 else 0))
    e = epc(f16)
    K = 2 * beam
    ld = (vocab + 7) // 8 * 8
    M = bsz * beam
    small = vocab * beam <= 128
    if small:      # every element may reach the list: all distinct, a quarter apart
        x = np.stack([rng.permutation(vocab) for _ in range(M)]).astype(np.float64) * 0.25 - 3.0
    else:
        x = rng.uniform(-3.0, 0.0, size=(M, vocab))
    cum = (-(0.31 * (np.arange(M) % beam) + 0.07 * (np.arange(M) // beam)) - rng.uniform(0, 0.2, M)).astype(np.float32)
    nb = 1 if step == 0 else beam
    nwin = 2 * K + SPARE              # a row that a NaN or cum = -inf takes out still leaves 2 * beam + 1 scripted scores
    deal = lambda j: int((j + s) % nb)     # noqa: E731
    vals = WIN_TOP - WIN_STEP * np.arange(nwin)
    for s in range(bsz):
        if small or place in ("constant_row", "identical_rows"):
            break
        r0 = s * beam
        chunk0 = int(rng.integers(64, 900))
        if place == "one_chunk":          # the K best in the 16 bytes one lane reads (and the same lane's chunk of the next rows)
            pos = [(b, chunk0 * e + j) for b in range(nb) for j in range(e)][:K]
            pos += [(0, (chunk0 + 200 + j) % 1000 * e) for j in range(SPARE)]      # the runners-up: row 0, other lanes
        elif place == "one_wave":         # distinct lanes of wave 3
            pos = [(deal(j), (192 + 5 * j % 64) * e + int(rng.integers(e))) for j in range(nwin)]
        elif place == "per_wave":         # one per wave, up to all 16
            pos = [(deal(j), (64 * (j % 16) + j) * e + int(rng.integers(e))) for j in range(min(nwin, 16))]
        elif place == "same_col":         # the same two columns in every beam row
            ca, cbb = int(rng.integers(3, vocab)), int(rng.integers(3, vocab - 1))
            cbb += cbb == ca
            pos = [(b, ca) for b in range(nb)] + [(b, cbb) for b in range(nb)]
        elif place == "rows_gt0":
            pos = [(1 + int(rng.integers(nb - 1)), int(c)) for c in rng.choice(np.arange(3, vocab), nwin, replace=False)]
        else:
            pos = [(deal(j), int(c)) for j, c in enumerate(rng.choice(np.arange(3, vocab), nwin, replace=False))]
            if place == "col0":
                pos[0], pos[3] = (0, 0), (nb - 1, 0)
            if place == "last_col":
                pos[0], pos[3] = (nb - 1, vocab - 1), (0, vocab - 1)
        seen = set()
        for (b, col), v in zip(pos, vals):
            if (b, col) in seen or col >= vocab:
                continue
            seen.add((b, col))
            x[r0 + b, col] = v
    if place == "constant_row":           # row 0 of every crop constant: its candidates tie, the lower token wins
        for s in range(bsz):
            x[s * beam] = 1.5
            cum[s * beam + 1:(s + 1) * beam] -= 8.0
    if place == "identical_rows":         # every row of a crop the same bits, cum equal: (beam, token) ties across the rows
        for s in range(bsz):
            x[s * beam:(s + 1) * beam] = x[s * beam]
            cols = rng.choice(np.arange(3, vocab), 3, replace=False)
            x[s * beam:(s + 1) * beam, cols] = (7.0, 6.0, 5.0)
            cum[s * beam:(s + 1) * beam] = cum[s * beam]
    if small and place == "on_pad":       # (the on_pad and on_eos cases are all small) the best logit of two rows sits on the masked column
        x[::beam, pad] = 9.0
        x[beam - 1::beam, pad] = 8.5
    if small and place == "on_eos":
        x[::beam, eos] = 9.0
        x[beam - 1::beam, eos] = 8.5
    big = 65504.0 if f16 else 1e30
    last = M - 1
    if special == "nan":                  # one NaN: the whole row is -inf (log_softmax of a row with a NaN)
        x[last, int(rng.integers(3, vocab))] = np.nan
    elif special == "nan_alone":          # ... also where the NaN shares its 16-byte chunk with nothing but -inf and padding
        x[last, 16] = np.nan
        x[0, 8:8 + e] = NINF
        x[0, 8] = np.nan
    elif special == "posinf":
        x[last, int(rng.integers(3, vocab))] = np.inf
    elif special == "neginf_row":
        x[last] = NINF
    elif special == "neginf_runs":        # runs of -inf chunks between finite ones, a thread's first chunk among them
        for r in range(M):
            for a in rng.integers(0, vocab // e - 40, 6):
                x[r, int(a) * e:(int(a) + int(rng.integers(1, 40))) * e] = NINF
            x[r, :2 * e] = NINF
            x[r, 1024 * e:1025 * e] = 4.0 + 0.125 * r       # thread 0: first chunk dead, second alive
    elif special == "cum_neginf":
        cum[last] = NINF
    elif special == "magnitude":
        x[last, 5], x[last, 6] = big, -big
        x[0, 7] = -big
        if not f16:       # the last row of every crop: 0 beside +1e30 and -1e30.  Its winner scores cum exactly (score_bound: lse = mx),
            for s in range(bsz):      # the zeros tie at -1e30 with equal bits; row 0 of the crop carries a -1e30 among finite logits
                r = (s + 1) * beam - 1
                x[r] = 0.0
                x[r, 5], x[r, 6] = big, -big
                x[s * beam, 7] = -big
    elif special == "step0_nan":          # step 0 reads row 0 of each crop and no cum
        for s in range(bsz):
            x[s * beam + 1:(s + 1) * beam] = np.nan
        cum[:] = np.nan
    elif special == "step0_decoys":       # ... nor rows that would win if they competed
        for s in range(bsz):
            x[s * beam + 1:(s + 1) * beam, 3:11] = 30.0 - np.arange(8)
        cum[:] = 50.0 + np.arange(M)
    L = np.empty((M, ld), np.float16 if f16 else np.float32)
    with np.errstate(over="ignore"):
        L[:, :vocab] = x
    for r in range(M):
        L[r, vocab:] = PADFILL[(r + seed) % 3]
    return {"f16": f16, "logits": L, "cum": cum, "step": step, "max_len": max_len, "min_len": min_len, "pad": pad, "eos": eos,
            "vocab": vocab, "ld": ld, "beam": beam, "bsz": bsz}


def reference(case):
    """candidates() of a case, cached on it"""
    if "_ref" not in case:
        case["_ref"] = candidates(case["logits"], case["cum"], case["step"], case["max_len"], case["min_len"], case["pad"],
                                  case["eos"], case["vocab"], case["beam"], case["bsz"])
    return case["_ref"]


def undecided_pairs(case):
    """adjacent pairs among the reference's first 2 * beam + 1 scores that are neither an exact tie nor 4 x score_bound apart"""
    bad = []
    K = 2 * case["beam"]
    for s, r in enumerate(reference(case)):
        o = r["order"][:K + 1]
        for a, b in zip(o[:-1], o[1:]):
            ga, gb = r["scores"][a], r["scores"][b]
            if ga == gb:
                if not tie_is_exact(case, s, int(a), int(b)):
                    bad.append((s, int(a), int(b), "tie between different operands"))
            elif not ga - gb >= 4 * max(r["bound"][a], r["bound"][b]):
                bad.append((s, int(a), int(b), float(ga - gb), float(max(r["bound"][a], r["bound"][b]))))
    return bad


# ------------------------------------------------------------------------------------------------- cases: the search
SEARCH = dict(vocab=24, ld=24, max_len=6, min_len=1, pad=1, eos=2)
SEARCH_SHAPES = [(beam, bsz) for beam in (1, 2, 3, 4) for bsz in (65, 1)]
KINDS = ("all_at_once", "one_per_step", "eos_low", "never")


def crop_kind(s, bsz, late=True):
    """crop 64, the first thread of beam_select's second block, is among the late ones; late=False: a batch that ends early"""
    if not late:
        return KINDS[s % 2]
    return "never" if s == 64 or bsz == 1 else KINDS[s % 4]


def make_search(beam, bsz, f16, seed=0, late=True):
    """Scripted logits [max_len + 1][bsz*beam][ld] (device type) of a batch whose crops end four ways: `beam` hypotheses finalised
    in one step (step 2) | one per step from step 1 | eos only at positions >= beam until the forced step | no eos candidate at
    all until step max_len (late=False: the first two ways only, so the search ends before max_len).  From the step after a crop finishes (by the free-running reference) its logits are NaN."""
    p = dict(SEARCH, beam=beam, bsz=bsz)
    V, ML, eos = p["vocab"], p["max_len"], p["eos"]
    rng = np.random.default_rng(500 + 10 * beam + bsz + seed)
    M = bsz * beam
    x = np.empty((ML + 1, M, V))
    free_cols = np.array([c for c in range(V) if c not in (eos, p["pad"])])
    for t in range(ML + 1):
        for r in range(M):      # a row's values fall from -2.5 in irregular steps of 0.35 .. 0.65: no two sums of steps coincide
            x[t, r, rng.permutation(V)] = -2.5 - np.concatenate(([0.0], np.cumsum(rng.uniform(0.35, 0.65, V - 1))))
            x[t, r, eos] = -30.0
    for s in range(bsz):
        kind = crop_kind(s, bsz, late)
        rows = slice(s * beam, (s + 1) * beam)
        if kind == "all_at_once":         # step 2: eos dominates every row -> the first `beam` candidates are all eos
            x[2, rows, eos] = 6.0
        elif kind == "one_per_step":      # from step 1: eos is the best continuation of the best row only
            for t in range(1, ML + 1):
                x[t, s * beam, eos] = 3.0
        elif kind == "eos_low":           # every row: `beam` tokens above its eos, so no eos among the first `beam` candidates
            for t in range(1, ML):
                for r in range(s * beam, (s + 1) * beam):
                    if r > s * beam:      # the rows behind the best one flat (steps of 0.035 .. 0.065): row 0's eos stays in the list
                        x[t, r] = -2.5 + 0.1 * (x[t, r] + 2.5)
                    v = np.sort(x[t, r, free_cols])[::-1]
                    x[t, r, eos] = 0.5 * (v[beam - 1] + v[beam])
    L = x.astype(np.float16 if f16 else np.float32)
    free = search(p, logits=L, dtype=np.float64)
    done_at = np.full(bsz, ML + 1)
    for t in range(free["steps"]):
        done_at = np.where((free["finished"][t] == 1) & (done_at > t), t, done_at)
    for s in range(bsz):
        L[done_at[s] + 1:, s * beam:(s + 1) * beam] = np.nan
    return p, L, done_at


def _lists(beam, bsz, ML, fill_tok=5):
    S = ML + 1
    cs = np.tile(-(np.arange(2 * beam, dtype=np.float32) + 1), (S, bsz, 1)) - np.arange(S, dtype=np.float32)[:, None, None]
    ct = np.full((S, bsz, 2 * beam), fill_tok, np.int32) + np.arange(2 * beam, dtype=np.int32)
    cb = np.tile(np.arange(2 * beam, dtype=np.int32) % beam, (S, bsz, 1))
    return cs, ct, cb


def list_cases():
    """Hand-written candidate lists [S][bsz][2 * beam] that reach what no decoder produces.  -> {name: (p, (scores, tokens, beams))}"""
    out = {}
    eos, pad, ML = 2, 1, 5
    # beam 3, three crops.  crop 0: four eos in the list of step 1 (two finalise, one slot becomes an ignored one), the ignored
    # slot's eos among the first `beam` at step 2, an eos scored -inf at step 2.  crop 1: nothing ever finalises.  crop 2: two
    # finalised hypotheses whose normalised scores are the same bits (-2 / 2 and -3 / 3), then a worse third.
    p = dict(vocab=24, ld=24, max_len=ML, min_len=1, pad=pad, eos=eos, beam=3, bsz=3)
    cs, ct, cb = _lists(3, 3, ML)
    ct[1, 0] = (eos, 7, eos, eos, eos, 9)
    cb[1, 0] = (2, 2, 2, 1, 0, 2)
    ct[2, 0] = (7, 8, eos, eos, 9, 10)           # slot 2 is the ignored one: its eos must not finalise; position 3 is not read
    cs[2, 0, 3] = NINF
    ct[3, 0] = (eos, 8, 9, 10, 11, 12)
    cs[3, 0, 0] = NINF                           # an eos with score -inf is no eos
    ct[4, 0] = (eos, eos, 9, 10, 11, 12)         # third hypothesis: the crop ends here; the second eos finds no slot left
    ct[1, 2], cs[1, 2, 0] = (eos, 7, 8, 9, 10, 11), -2.0
    ct[2, 2], cs[2, 2, 1] = (7, eos, 8, 9, 10, 11), -3.0
    ct[3, 2], cs[3, 2, 0] = (eos, 7, 8, 9, 10, 11), -8.0
    out["ignore-inf-ties-never"] = (p, (cs, ct, cb))
    # beam 4, two crops: every beam from one parent at every step (crop 0), the parents reversed at every step (crop 1), eos at
    # positions beam .. 2 * beam - 1 only
    p = dict(p, beam=4, bsz=2)
    cs, ct, cb = _lists(4, 2, ML)
    cb[:, 0] = 3
    cb[1::2, 0] = 1
    cb[:, 1] = (3, 2, 1, 0, 0, 1, 2, 3)
    ct[:, :, 5] = eos
    out["one-parent-reversal"] = (p, (cs, ct, cb))
    # beam 2: more eos than slots in one list of the very first step; beam 1: the smallest state
    p = dict(p, beam=2, bsz=2)
    cs, ct, cb = _lists(2, 2, ML)
    ct[0, 0] = (eos, eos, eos, 7)
    ct[0, 1] = (7, eos, eos, eos)
    ct[1, 1] = (eos, 8, 9, 10)                   # slot 1 was filled with an ignored eos: position 1 is masked, 0 finalises
    ct[2, 1] = (8, eos, 9, 10)
    out["more-eos-than-slots"] = (p, (cs, ct, cb))
    p = dict(p, beam=1, bsz=2)
    cs, ct, cb = _lists(1, 2, ML)
    ct[3, 0, 0] = eos
    ct[:, 1, 1] = eos
    out["beam1"] = (p, (cs, ct, cb))
    return out
