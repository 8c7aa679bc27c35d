"""CPU checks of oracle/beam_ref.py, the reference, bound and cases of tests/test_beam_gpu.py.

* The restated bookkeeping (select / ancestry / best), fed the candidate lists the torch oracle traced on a small synthetic
  model, returns that oracle's tokens, scores, finalised score lists and step count exactly.
* ``candidates`` is F.log_softmax in fp64 with the generator's masks, NaN, +inf and all -inf rows included.
* Every case decides: adjacent pairs among the reference's first 2 * beam + 1 scores are exact ties the device sees as equal bits,
  or at least 4 x score_bound apart — so the GPU test may demand the exact list.
* An fp32 emulation of beam_candidates_kernel (chunking, running maximum, merge order, 64-bit keys, three selection stages)
  returns the exact lists with every score inside score_bound, on every case.
* The same emulation with one seeded bug at a time, and the bookkeeping with one mutated, must change what the GPU test compares
  on at least one named case; the test prints which cases catch which bug.

Measured here (libm's exp2 and log in the place of the hardware's): the clean emulation's worst max err / bound is 0.16 with f16
logits and 0.17 with fp32.  Each candidates bug runs on the cases built for it (WHERE below) and on every 17th case of the table,
not on all of them: the module stays quick, and a bug that only an unrelated case caught would be caught by accident.
    min_len_if is caught only by the CPU-only case with min_len 9 > max_len 6: the kernel itself applies the two masks as independent
    ifs, both entries and mhip_trocr_create refuse that configuration, so on the device the refusal test stands guard for it.
    nan_chunk_skipped is the kernel's behaviour before this reference existed (the nan_alone cases).
"""
import numpy as np
import pytest

from oracle import beam_ref as R

PARAMS = R.case_params()
_CASES = {}


def _case(f16, pid, kw):
    if (f16, pid) not in _CASES:
        c = R.make_case(f16, **kw)
        R.reference(c)
        _CASES[(f16, pid)] = c
    return _CASES[(f16, pid)]


def _verdict(case, cs, ct, cb):
    """what tests/test_beam_gpu.py asserts of one launch -> (lists equal, max err / bound, no NaN, -inf where the reference has it)"""
    ref = R.reference(case)
    K = 2 * case["beam"]
    equal, ratio, clean = True, 0.0, True
    for s, r in enumerate(ref):
        equal &= bool(np.array_equal(ct[s], r["cand_tokens"]) and np.array_equal(cb[s], r["cand_beams"]))
        clean &= not np.isnan(cs[s]).any() and bool((cs[s][1:] <= cs[s][:-1]).all())
        inf = r["cand_scores"] == R.NINF
        clean &= bool((cs[s][inf] == R.NINF).all()) and bool(np.isfinite(cs[s][~inf]).all())
        if equal and clean and (~inf).any():
            err = np.abs(cs[s][~inf].astype(np.float64) - r["cand_scores"][~inf])
            ratio = max(ratio, float((err / r["bound"][r["order"][:K]][~inf]).max()))
    return equal, ratio, clean


# ------------------------------------------------------------------------------------------------ the reference is the operation
def test_bookkeeping_agrees_with_the_torch_oracle():
    from marie_icr_amd.weights import make_image_u8, make_trocr_state
    from oracle.trocr_torch import TorchTrocrOracle

    enc, dec, vocab, maxpos, img = (128, 2, 4), (192, 2, 4, 384), 61, 24, 64
    st = make_trocr_state(3, enc, dec, vocab, maxpos, img=img)
    crops = make_image_u8(5, 4, img, img)
    for beam, max_len_b in ((3, 9), (1, 5), (4, 12)):
        o = TorchTrocrOracle(st, enc[2], dec[2], beam=beam, max_len_b=max_len_b, img=img)
        hyp, tr = o.generate(crops, want_trace=True)
        K, S = 2 * beam, tr["scores"].shape[0]
        p = dict(vocab=vocab, ld=64, max_len=o.max_len, min_len=1, pad=1, eos=2, beam=beam, bsz=len(crops))
        lists = (tr["scores"][:, :, :K].astype(np.float32), tr["tokens"][:, :, :K].astype(np.int32), tr["beams"][:, :, :K].astype(np.int32))
        got = R.search(p, lists=tuple(np.concatenate([a, a[-1:]]) for a in lists))       # free to run on: it must stop by itself
        assert got["steps"] == S, (beam, got["steps"], S)
        for s, (toks, score) in enumerate(hyp):
            n = int(got["out_len"][s])
            assert n == len(toks) and np.array_equal(got["out_tokens"][s, :n], toks)
            assert np.float32(score) == got["out_score"][s]                            # float(f32) / (step + 1) in fp64, then fp32: the same bits
            fin = np.asarray(tr["finalized"][s], np.float64).astype(np.float32).reshape(-1)
            assert np.array_equal(got["fin_score"][s * beam:s * beam + int(got["fin_count"][-1, s])], fin)
        assert np.array_equal(got["finished"].astype(bool), ~np.concatenate([tr["active"][1:], np.zeros((1, len(crops)), bool)]))


@pytest.mark.parametrize("step,max_len,min_len", [(0, 6, 1), (1, 6, 1), (2, 6, 3), (6, 6, 1), (7, 6, 1)])
def test_candidates_are_log_softmax_with_the_generators_masks(step, max_len, min_len):
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(step)
    beam, bsz, vocab, pad, eos = 3, 4, 29, 1, 2
    x = rng.normal(0, 3, (bsz * beam, 32)).astype(np.float32)
    x[1, 7], x[4, 3], x[6, :] = np.nan, np.inf, -np.inf
    x[9, 5:20] = -np.inf
    cum = rng.normal(-2, 1, bsz * beam).astype(np.float32)
    lp = F.log_softmax(torch.from_numpy(x[:, :vocab].astype(np.float64)), dim=-1)
    lp[lp != lp] = -np.inf
    lp[:, pad] = -np.inf
    if step >= max_len:
        lp[:, :eos] = -np.inf
        lp[:, eos + 1:] = -np.inf
    elif step < min_len:
        lp[:, eos] = -np.inf
    lp = lp.view(bsz, beam, -1)
    flat = (lp[:, :1] if step == 0 else lp + torch.from_numpy(cum.astype(np.float64)).view(bsz, beam, 1)).reshape(bsz, -1)
    order = torch.argsort(flat, dim=1, descending=True, stable=True)
    got = R.candidates(x, cum, step, max_len, min_len, pad, eos, vocab, beam, bsz)
    for s, r in enumerate(got):
        want = flat[s].numpy()
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(r["scores"])) and (r["scores"][~fin] == -np.inf).all()
        assert np.abs(r["scores"][fin] - want[fin]).max(initial=0.0) <= 1e-12
        o = order[s, :2 * beam].numpy()
        assert np.array_equal(r["cand_tokens"], o % vocab) and np.array_equal(r["cand_beams"], o // vocab)


# ------------------------------------------------------------------------------------------------------- the cases are sharp
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_every_case_decides(f16):
    for pid, kw in PARAMS:
        assert R.undecided_pairs(_case(f16, pid, kw)) == [], pid
    for beam, bsz in R.SEARCH_SHAPES:
        p, L, done_at = R.make_search(beam, bsz, f16)
        free = R.search(p, logits=L, dtype=np.float64)
        for t in range(free["steps"]):
            cum = np.zeros(bsz * beam) if t == 0 else free["cum"][t - 1]
            case = dict(p, f16=f16, logits=L[t], cum=np.nan_to_num(cum).astype(np.float32), step=t)
            R.reference(case)
            live = [s for s in range(bsz) if done_at[s] >= t]
            bad = [b for b in R.undecided_pairs(case) if b[0] in live]
            assert bad == [], (beam, bsz, t, bad[:3])


def test_cases_cover_what_the_kernel_branches_on():
    ids = [p for p, _ in PARAMS]
    assert len(set(ids)) == len(ids)
    for beam in (1, 2, 3, 4):
        vs = {kw["vocab"] for _, kw in PARAMS if kw["beam"] == beam}
        assert {2 * beam, 8, 9, 17, 4095, 4096, 4097, 8191, 8192, 8193} <= vs
        assert {kw["bsz"] for _, kw in PARAMS if kw["beam"] == beam} >= {1, 3}
    assert {(kw["beam"], kw["bsz"]) for _, kw in PARAMS if kw["vocab"] == 50265} == {(3, 2), (4, 2)}
    for f16 in (True, False):
        e = R.epc(f16)
        kw = dict(next(kw for p, kw in PARAMS if kw["place"] == "one_chunk" and kw["beam"] == 4))
        c = _case(f16, R.case_id(kw), kw)
        for s, r in enumerate(R.reference(c)):      # the eight winners: one lane (chunk index mod 1024)
            top = r["order"][:8]
            assert len({(int(t) % c["vocab"]) // e % 1024 for t in top}) == 1
        kw = dict(next(kw for p, kw in PARAMS if kw["place"] == "one_wave" and kw["beam"] == 4))
        c = _case(f16, R.case_id(kw), kw)
        for r in R.reference(c):
            lanes = [(int(t) % c["vocab"]) // e % 1024 for t in r["order"][:8]]
            assert {l // 64 for l in lanes} == {3} and len(set(lanes)) == 8
        kw = dict(next(kw for p, kw in PARAMS if kw["place"] == "per_wave" and kw["beam"] == 4))
        c = _case(f16, R.case_id(kw), kw)
        for r in R.reference(c):
            assert len({(int(t) % c["vocab"]) // e % 1024 // 64 for t in r["order"][:8]}) == 8
        kw = dict(next(kw for p, kw in PARAMS if kw["place"] == "rows_gt0" and kw["beam"] == 3))
        assert all((r["cand_beams"] > 0).all() for r in R.reference(_case(f16, R.case_id(kw), kw)))
        kw = dict(next(kw for p, kw in PARAMS if kw["place"] == "same_col" and kw["beam"] == 4))
        for r in R.reference(_case(f16, R.case_id(kw), kw)):
            assert sorted(r["cand_beams"].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3] and len(set(r["cand_tokens"].tolist())) == 2
        kw = dict(next(kw for p, kw in PARAMS if kw["place"] == "constant_row" and kw["beam"] == 2))
        for r in R.reference(_case(f16, R.case_id(kw), kw)):
            assert r["cand_tokens"].tolist() == [0, 2, 3, 4] and r["cand_beams"].tolist() == [0] * 4       # pad = 1 skipped
        kw = dict(next(kw for p, kw in PARAMS if kw["step"] == 6 and kw["beam"] == 3))
        for r in R.reference(_case(f16, R.case_id(kw), kw)):
            assert r["cand_tokens"].tolist()[:3] == [2, 2, 2] and r["cand_tokens"].tolist()[3:] == [0, 1, 3]
            assert np.isfinite(r["cand_scores"][:3]).all() and (r["cand_scores"][3:] == -np.inf).all()


def test_search_scripts_end_the_four_ways():
    for beam, bsz in R.SEARCH_SHAPES:
        p, L, done_at = R.make_search(beam, bsz, True)
        free = R.search(p, logits=L, dtype=np.float64)
        ML, eos = p["max_len"], p["eos"]
        for s in range(bsz):
            kind = R.crop_kind(s, bsz)
            fc = free["fin_count"][:, s]
            if kind == "all_at_once":
                assert done_at[s] == 2 and fc[1] == 0 and fc[2] == beam
            elif kind == "one_per_step":
                assert done_at[s] == beam and list(fc[:beam + 1]) == list(range(beam + 1))
            else:
                assert done_at[s] == ML and fc[ML - 1] == 0 and fc[ML] == beam
                seen = [(free["cand_tokens"][t, s] == eos) & np.isfinite(free["cand_scores"][t, s]) for t in range(ML)]
                assert not any(m[:beam].any() for m in seen)
                assert any(m.any() for m in seen) == (kind == "eos_low")
        if bsz == 65:
            assert R.crop_kind(64, bsz) == "never" and free["steps"] == ML + 1
            assert np.isnan(L[3, 0]).all() and not np.isnan(L[2, :beam]).any()             # crop 0 finished at step 2


def test_hand_written_lists_reach_what_no_decoder_produces():
    cases = R.list_cases()
    p, lists = cases["ignore-inf-ties-never"]
    tr = R.search(p, lists=lists)
    assert tr["ignore"][1, 0:3].tolist() == [0, 0, 1]                 # four eos in a list of six: one ignored slot
    assert tr["fin_count"][:, 0].tolist()[:5] == [0, 2, 2, 2, 3]      # the ignored slot's eos (step 2) and the -inf eos (step 3) are none
    assert tr["out_len"][1] == 0 and tr["out_score"][1] == -np.inf and (tr["out_tokens"][1] == p["pad"]).all()
    assert tr["fin_score"][6] == tr["fin_score"][7] == np.float32(-1) and tr["out_len"][2] == 2       # -2 / 2 == -3 / 3: the first
    p, lists = cases["one-parent-reversal"]
    tr = R.search(p, lists=lists)
    assert (tr["parent"][2, :4] == 3).all() and (tr["parent"][1, :4] == 1).all() and tr["parent"][1, 4:].tolist() == [7, 6, 5, 4]
    assert tr["fin_count"][:p["max_len"]].max() == 0                  # eos at position 5 of 8: neither finalised nor active
    assert not (tr["last_tok"][:p["max_len"]] == p["eos"]).any()
    p, lists = cases["more-eos-than-slots"]
    tr = R.search(p, lists=lists)
    assert tr["finished"][0].tolist() == [1, 0] and tr["ignore"][0, 2:4].tolist() == [0, 1] and tr["fin_count"][0].tolist() == [2, 1]


# ------------------------------------------------------------------------------------------- the emulation and its mutations
_EMU = {}


def _emulated(f16, pid, kw, mut=None):
    key = (f16, pid, mut)
    if key not in _EMU:
        _EMU[key] = _verdict(_case(f16, pid, kw), *R.emulate_candidates(_case(f16, pid, kw), mut))
    return _EMU[key]


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_clean_emulation_returns_the_exact_lists_inside_the_bound(f16):
    worst = (0.0, None)
    for pid, kw in PARAMS:
        equal, ratio, clean = _emulated(f16, pid, kw)
        assert equal and clean and ratio <= 1.0, (pid, equal, ratio, clean)
        worst = max(worst, (ratio, pid))
    print(f"{'f16' if f16 else 'f32'}: clean emulation, worst max err / bound {worst[0]:.3f} at {worst[1]}")


# the cases built to catch each candidates bug
WHERE = {
    "tie_high_index": lambda kw: kw["place"] in ("constant_row", "identical_rows") or kw["step"] >= kw["max_len"],
    "shortlist_k_minus_1": lambda kw: kw["place"] == "one_chunk" or kw["vocab"] <= 9,
    "drop_wave_partial": lambda kw: kw["vocab"] in (4097, 8193) and kw["place"] == "spread" and not kw["special"],
    "padding_in_max": lambda kw: kw["vocab"] in (9, 17, 4095) and kw["place"] == "spread" and not kw["special"],
    "pad_unmasked": lambda kw: kw["place"] == "on_pad",
    "beam_rows_at_step0": lambda kw: kw["step"] == 0,
    "cum_at_step0": lambda kw: kw["step"] == 0,
    "inf_chunk_nan": lambda kw: kw["special"] == "neginf_runs",
    "nan_chunk_skipped": lambda kw: kw["special"] == "nan_alone",
}


def test_every_seeded_bug_changes_a_named_case():
    uncaught = []
    cpu_only = [(R.case_id(kw) + "-minlen9", kw) for kw in R.CPU_ONLY_CASES]
    for mut in R.CAND_MUTATIONS:
        caught = []
        built = [(pid, kw) for i, (pid, kw) in enumerate(PARAMS) if kw["vocab"] < 10000 and (i % 17 == 0 or WHERE.get(mut, bool)(kw))]
        for f16 in (True, False):
            for pid, kw in (cpu_only if mut == "min_len_if" else built):
                equal, ratio, clean = _emulated(f16, pid, kw, mut)
                if not (equal and clean and ratio <= 1.0):
                    caught.append(("f16/" if f16 else "f32/") + pid)
        print(f"{mut}: caught by {len(caught)} cases, e.g. {caught[:4]}")
        if not caught:
            uncaught.append(mut)
    searches = [(f"search-beam{b}-bsz{n}", R.make_search(b, n, True)[:2]) for b, n in R.SEARCH_SHAPES if n == 1 or b == 3]
    lists = R.list_cases()
    for mut in R.STATE_MUTATIONS:
        caught = []
        for name, (p, ls) in lists.items():
            clean = R.search(p, lists=ls)
            bad = R.search(p, lists=ls, steps=clean["steps"], mut=mut)
            if R.differing(R.compared(clean, p["beam"]), R.compared(bad, p["beam"])):
                caught.append(name)
        for name, (p, L) in searches:
            clean = R.search(p, logits=L, dtype=np.float64)
            ls = (clean["cand_scores"].astype(np.float32), clean["cand_tokens"], clean["cand_beams"])
            forced = R.search(p, lists=ls, steps=clean["steps"])
            bad = R.search(p, lists=ls, steps=clean["steps"], mut=mut)
            if R.differing(R.compared(forced, p["beam"]), R.compared(bad, p["beam"])):
                caught.append(name)
        print(f"{mut}: caught by {caught}")
        if not caught:
            uncaught.append(mut)
    assert not uncaught, uncaught
