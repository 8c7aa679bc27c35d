"""CPU checks of oracle/cross_attention_ref.py, the fp64 references, derived bounds, kernel emulation and operand sets of
tests/test_cross_attention_gpu.py: the references are softmax attention and fairseq's MultiheadAttention, the emulation of the
kernel's arithmetic stays within the derived cross_attn bound on every case, every likely kernel bug moves the reference of
every case it applies to by at least ten times the bound — so a kernel with any of these bugs cannot pass the GPU test — the
softmax trajectories the variants promise happen, and the case table covers every instantiation against every ring edge."""
import functools

import numpy as np
import pytest

from oracle import cross_attention_ref as R

ALL = R.all_params()
IDS = [p for p, _ in ALL]


@functools.lru_cache(maxsize=None)
def _judged(pid):
    """per case, computed once: emulation error / bound ratios and how far each mutation moves its reference, in bounds"""
    case = R.make_case(**dict(ALL)[pid])
    qt = R.f16(R.qt_stage(case)[0])                      # the CPU's stand-in for the device's absorbed queries
    ct = R.emulate(case, qt)
    st = R.stages(case, qt, ct, e2e=False)
    err = np.abs(ct - st["ct_ref"])
    moves = {name: R.moved(m, st[stage + "_ref"], st[stage + "_hard"]) for name, (stage, m) in R.mutations(case, qt, ct).items()}
    return {"finite": bool(np.isfinite(ct).all()), "hard": float((err / st["ct_hard"]).max()),
            "mean": float(err.mean() / st["ct_mean"].mean()), "moves": moves}


def test_reference_is_softmax_attention():
    """ct_stage against an independent restatement: exp, one (row, head) at a time"""
    case = R.make_case(ed=256, beam=2, heads=4, n_keys=45, crops=2, kv_extra=8, seed=1)
    rng = np.random.default_rng(0)
    qt = rng.normal(0, 0.2, (4, 4, 256))
    got = R.ct_stage(case, qt)
    for r in range(4):
        rows = case["E"][r // 2, :45].astype(np.float64)
        for h in range(4):
            s = rows @ qt[r, h] * np.log(2.0)
            p = np.exp(s - s.max())
            p /= p.sum()
            np.testing.assert_allclose(got["ref"][r, h], p @ rows, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(got["p"][r, h], p, rtol=1e-11, atol=1e-15)
            assert (got["hard"][r, h] >= got["mean"][r, h]).all() and (got["mean"][r, h] > 0).all()


def test_end_to_end_reference_is_fairseq_attention_and_the_absorbed_form_equals_it():
    case = R.make_case(ed=256, beam=3, heads=4, n_keys=70, crops=2, kv_extra=0, seed=2)
    q, E, wk, wv, bk, bv = (case[k].astype(np.float64) for k in ("q", "E", "wk", "wv", "bk", "bv"))
    ref = R.fairseq_reference(case)
    for r in range(6):
        K, V = E[r // 3, :70] @ wk.T + bk, E[r // 3, :70] @ wv.T + bv
        for h in range(4):
            sl = slice(64 * h, 64 * h + 64)
            s = K[:, sl] @ q[r, sl]
            p = np.exp(s - s.max())
            np.testing.assert_allclose(ref[r, sl], (p / p.sum()) @ V[:, sl], rtol=1e-12, atol=1e-13)
    # q . b_k is constant over the keys: dropping it changes nothing
    np.testing.assert_allclose(R.fairseq_reference(case, with_bk=False), ref, rtol=1e-11, atol=1e-12)
    # the absorbed form with unrounded intermediates: qt = log2 e W_k,h^T q_h, softmax2 over E, W_v,h ct + b_v
    qt = np.einsum("rhj,hjd->rhd", q.reshape(6, 4, 64), wk.reshape(4, 64, 256)) * np.log2(np.e)
    ct = R.ct_stage(case, qt)["ref"]
    np.testing.assert_allclose(R.ao_stage(case, ct)[0], ref, rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize("pid", IDS)
def test_emulated_kernel_arithmetic_stays_within_the_context_bound(pid):
    j = _judged(pid)
    assert j["finite"]
    assert j["hard"] <= 1.0, (pid, j["hard"])
    assert j["mean"] <= 1.0, (pid, j["mean"])


@pytest.mark.parametrize("pid", IDS)
def test_each_kernel_bug_moves_the_reference_by_ten_bounds(pid):
    kw = dict(ALL)[pid]
    n, v = kw["n_keys"], kw["variant"]
    moves = _judged(pid)["moves"]
    want = set()
    if kw["kv_extra"] or (n % 8) or kw["crops"] > 1:
        want.add("admit_key_n")
    if kw["heads"] >= 2:
        want.add("swap_heads_0_1")
    if kw["crops"] >= 2:
        want.add("crop0_E_for_all")
    if v is None:
        if n >= 2:
            want |= {"drop_last_key"} | ({"beam0_queries_for_all"} if kw["beam"] >= 2 else set())
    elif v in ("late_dominant", "shift_plus", "shift_minus", "shift_zero"):
        want |= {"drop_last_key", "no_rescale_branch", "rescale_without_scaling"}
    elif v == "rising":
        want |= {"no_rescale_branch", "rescale_without_scaling"}
    assert want <= set(moves), (pid, want - set(moves))
    for name, m in moves.items():
        assert m >= 10.0, (pid, name, m)


def test_every_mutation_is_exercised_somewhere_for_every_width_and_beam():
    names = {"drop_last_key", "drop_first_key", "drop_key_31", "drop_key_32", "admit_key_n", "swap_heads_0_1", "beam0_queries_for_all",
             "crop0_E_for_all"}
    for ed in R.EDS:
        have = set()
        for pid, kw in R.sweep_params():
            if kw["ed"] == ed:
                have |= set(_judged(pid)["moves"])
        assert names <= have, (ed, names - have)
        tr = set()
        for pid, kw in R.variant_params():
            if kw["ed"] == ed:
                tr |= set(_judged(pid)["moves"])
        assert {"no_rescale_branch", "rescale_without_scaling"} <= tr


@pytest.mark.parametrize("pid", [p for p, _ in R.variant_params()])
def test_softmax_trajectories_happen(pid):
    case = R.make_case(**dict(ALL)[pid])
    R.assert_trajectory(case, R.f16(R.qt_stage(case)[0]))
    if case["variant"] == "shift_plus":              # the shift moves only component ed - 1 of qt and nothing of the result
        zero = R.make_case(**dict(ALL)[pid.replace("shift_plus", "shift_zero")])
        np.testing.assert_array_equal(zero["E"], case["E"])
        a, b = R.qt_stage(case)[0], R.qt_stage(zero)[0]
        np.testing.assert_array_equal(a[..., :-1], b[..., :-1])
        assert (np.abs(a[..., -1] - R.SHIFT) <= 0.5).all() and (b[..., -1] == 0).all()
        np.testing.assert_allclose(R.ct_stage(case, a)["ref"], R.ct_stage(zero, b)["ref"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("pid", [p for p, _ in R.variant_params() + R.rows68_params()])
def test_emulated_chain_stays_within_the_end_to_end_bound(pid):
    case = R.make_case(**dict(ALL)[pid])
    qt = R.f16(R.qt_stage(case)[0])
    ct = R.emulate(case, qt)
    st = R.stages(case, qt, ct)
    out = R.f16(st["ao_ref"])
    err = np.abs(out - st["e2e_ref"])
    assert (err <= st["e2e_hard"]).all() and err.mean() <= st["e2e_mean"].mean()


def test_targets_carry_weight_and_operands_differ_between_crops_and_beams():
    for pid, kw in R.sweep_params():
        if kw["n_keys"] < 2 or kw["ed"] != 256:
            continue
        case = R.make_case(**kw)
        p = R.ct_stage(case, R.f16(R.qt_stage(case)[0]))["p"]
        w = np.take_along_axis(p, case["targets"][..., None], -1)[..., 0]
        assert 0.2 <= np.median(w) <= 0.95, (pid, np.median(w))
        if kw["crops"] > 1:
            assert not np.array_equal(case["E"][0], case["E"][1])
        if kw["beam"] > 1:
            q = case["q"].reshape(kw["crops"], kw["beam"], -1)
            assert not np.array_equal(q[:, 0], q[:, 1])
        pad = case["E"][:, kw["n_keys"]:]
        assert np.isfinite(case["E"]).all() and (pad.size == 0 or np.abs(pad).max() > 1.0)


def test_ring_rule_restated():
    assert [R.depth(ed, w) for ed in R.EDS for w in R.BEAMS] == [5] * 4 + [3] * 4 + [2] * 4 + [1] * 4
    assert {(ed, w) for ed in R.EDS for w in R.BEAMS if R.short_wave(ed, w)} == {(256, 3), (512, 3), (1024, 3)}


def test_case_table_covers_every_instantiation_against_every_ring_edge():
    sweep = [kw for _, kw in R.sweep_params()]
    assert len(set(IDS)) == len(IDS)
    for ed in R.EDS:
        d = R.depth(ed)
        classes = set(R.n_keys_classes(ed).values())
        assert {1, 31, 32, 33, 32 * d, 32 * d + 1, 32 * (d + 1) + 1, 577} == classes
        for beam in R.BEAMS:
            mine = [kw for kw in sweep if kw["ed"] == ed and kw["beam"] == beam]
            assert {kw["n_keys"] for kw in mine} == classes, (ed, beam)
            nts = {R.ntiles(kw["n_keys"]) for kw in mine}
            assert 1 in nts and d in nts and d + 1 in nts and d + 2 in nts and 19 in nts       # single tile; no / one / two feeding tiles
            assert d == 1 or any(t < d for t in nts)
            if R.short_wave(ed, beam):
                assert any(t <= d for t in nts) and any(t > d for t in nts)
        mine = [kw for kw in sweep if kw["ed"] == ed]
        assert {kw["heads"] for kw in mine} == set(R.HEADS)
        assert {kw["crops"] for kw in mine} == {1, 2, 3}
        assert {kw["kv_extra"] for kw in mine} == {0, 8}
        big = [kw for _, kw in R.rows68_params() if kw["ed"] == ed]
        assert len(big) == 1 and big[0]["crops"] * big[0]["beam"] == 68
        assert [kw["variant"] for _, kw in R.variant_params() if kw["ed"] == ed] == list(R.VARIANTS)
        iso = [kw for _, kw in R.isolation_params() if kw["ed"] == ed]
        assert any(kw["beam"] == 3 and kw["n_keys"] == 577 for kw in iso) and all(kw["crops"] >= 2 for kw in iso)
    assert all(kw["n_keys"] <= 577 and kw["crops"] * kw["beam"] <= 68 for _, kw in ALL + R.isolation_params())
