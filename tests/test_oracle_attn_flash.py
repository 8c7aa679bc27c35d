"""CPU checks of oracle/attn_flash_ref.py, the fp64 references, derived bounds, kernel emulation and operand sets of
tests/test_attn_flash_gpu.py: the reference equals softmax attention (with LayoutLMv3's bias and mask) restated one row at a time,
the emulation of the f16 kernel's arithmetic stays within the derived bound on every case, every named kernel bug moves the
reference of every case it applies to by at least ten times the bound — so a kernel with any of these bugs cannot pass the GPU
test — the softmax trajectories the variants promise happen, the case table covers every listed edge, and the block remap is a
bijection."""
import functools

import numpy as np
import pytest

from oracle import attn_flash_ref as R

ALL = R.all_params()
IDS = [p for p, _ in ALL]
TABLE = dict(ALL)


@functools.lru_cache(maxsize=None)
def _judged(pid):
    """per case, computed once: emulation error / bound ratios and how far each mutation moves its reference, in bounds"""
    case = R.build((pid, TABLE[pid]))
    ref = R.reference(case)
    em = R.emulate(case)
    err = np.abs(em - ref["ref"])
    moves = {name: R.moved(m, ref["ref"], ref["hard"]) for name, m in R.mutations(case).items() if (pid, name) not in R.NOT_JUDGED}
    h32 = {"hard": ref["hard32"], "mean": ref["mean32"]}
    return {"finite": bool(np.isfinite(em).all()), "hard": float((err / ref["hard"]).max()),
            "mean": float(err.mean() / ref["mean"].mean()), "moves": moves,
            "fp32_bound_is_tighter": bool((h32["hard"] <= ref["hard"]).all() and (h32["mean"] <= ref["mean"]).all()
                                          and (h32["mean"] <= h32["hard"]).all() and (ref["mean"] <= ref["hard"]).all())}


def _one_row_at_a_time(case, img, h, qi):
    """softmax(q . k ln 2 + bias ln 2 + mask) v for one query, natural exponentials, the buckets from the differences themselves"""
    import torch
    from layoutlmv3_ref import relative_position_bucket

    n, npq, npk = case["n_keys"], case["npad_q"], case["npad_k"]
    sl = slice(h * 64, h * 64 + 64)
    q = case["q"][img * npq + qi, sl].astype(np.float64)
    K = case["k"][img * npk:img * npk + n, sl].astype(np.float64)
    ldv = case["images"] * npk
    V = np.stack([case["vt"][(h * 64 + d) * ldv + img * npk:(h * 64 + d) * ldv + img * npk + n] for d in range(64)], 1).astype(np.float64)
    s = K @ q
    b = case["bias"]
    if b is not None:
        qc, kc = b["qcode"][img * npq + qi], b["kcode"][img * npk:img * npk + n]
        scale = float(R.SCALE_F32)
        for f, w, bins, maxd in ((0, b["w1"], R.BINS_1D, b["max_1d"]), (1, b["wx"], R.BINS_2D, b["max_2d"]), (2, b["wy"], R.BINS_2D, b["max_2d"])):
            bk = relative_position_bucket(torch.from_numpy(kc[:, f].astype(np.int64) - int(qc[f])), bins, maxd).numpy()
            s = s + w[h].astype(np.float64)[bk] * scale
        s = np.where(kc[:, 3] == 0, -np.inf, s)
    p = np.exp((s - s.max()) * np.log(2.0))
    p /= p.sum()
    return p @ V, p


@pytest.mark.parametrize("pid", [IDS[2], [p for p in IDS if p.startswith("split-i3") and "k193" in p][0],
                                 [p for p in IDS if "-b511x1000-mask_first_tile" in p][0],
                                 [p for p in IDS if "-b7x9-mask_middle_tile" in p][0]])
def test_reference_is_softmax_attention_one_row_at_a_time(pid):
    case = R.build((pid, TABLE[pid]))
    got = R.reference(case)
    rng = np.random.default_rng(3)
    for _ in range(24):
        img, h, qi = int(rng.integers(case["images"])), int(rng.integers(case["heads"])), int(rng.integers(case["n_queries"]))
        want, p = _one_row_at_a_time(case, img, h, qi)
        np.testing.assert_allclose(got["ref"][img, qi, h * 64:h * 64 + 64], want, rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(got["p"][img, h, qi], p, rtol=1e-10, atol=1e-15)
    assert (got["hard"] >= got["mean"]).all() and (got["mean"] > 0).all()


@pytest.mark.parametrize("pid", IDS)
def test_emulated_kernel_arithmetic_stays_within_the_bound(pid):
    j = _judged(pid)
    assert j["finite"]
    assert j["hard"] <= 1.0, (pid, j["hard"])
    assert j["mean"] <= 1.0, (pid, j["mean"])
    assert j["fp32_bound_is_tighter"]


@pytest.mark.parametrize("pid", IDS)
def test_each_kernel_bug_moves_the_reference_by_ten_bounds(pid):
    kw = TABLE[pid]
    n, nq, v = kw["n_keys"], kw["n_queries"], kw["variant"]
    moves = _judged(pid)["moves"]
    want = {"admit_key_n"}
    if kw["heads"] >= 2:
        want.add("swap_heads_0_1")
    if kw["images"] >= 2:
        want.add("image0_kv_for_all")
    if v is None:
        if n >= 2 and kw["bias"] is None:
            want.add("drop_last_key")
        if n >= 2 and nq >= 32:
            want.add("swap_query_tiles")
        if kw["bias"] is not None:
            want |= {"bias_table_p_dropped", "bias_table_x_dropped", "bias_table_y_dropped", "mask_ignored"}
    elif v in ("late_dominant", "shift_plus", "shift_minus", "shift_zero"):
        want |= {"drop_last_key", "no_branch", "no_scaling"}
    elif v in ("rising", "split_wave"):
        want |= {"no_branch", "no_scaling"}
    want -= {name for (p, name) in R.NOT_JUDGED if p == pid}
    assert want <= set(moves), (pid, want - set(moves))
    for name, m in moves.items():
        assert m >= 10.0, (pid, name, m)


def test_every_mutation_is_judged_somewhere_and_none_is_excused_everywhere():
    names = {"drop_last_key", "drop_first_key", "drop_key_63", "drop_key_64", "admit_key_n", "image0_kv_for_all", "swap_heads_0_1",
             "swap_query_tiles", "no_branch", "no_scaling", "bias_table_p_dropped", "bias_table_x_dropped", "bias_table_y_dropped",
             "mask_ignored"}
    have = {}
    for pid in IDS:
        for name in _judged(pid)["moves"]:
            have.setdefault(name, []).append(pid)
    assert names == set(have), names ^ set(have)
    for layout in ("fused", "split"):          # the key-dropping and admitting bugs are judged in both layouts
        for name in ("drop_last_key", "drop_first_key", "drop_key_63", "drop_key_64", "admit_key_n", "swap_query_tiles"):
            assert any(p.startswith(layout) for p in have[name]), (layout, name)
    assert all(p in TABLE and name in names for p, name in R.NOT_JUDGED)
    # the biased form's own bugs, the plain bugs on a biased case too
    biased = [p for p, kw in ALL if kw["bias"] is not None]
    for name in ("drop_last_key", "drop_key_64", "admit_key_n", "no_branch", "no_scaling", "mask_ignored"):
        assert any(p in biased for p in have[name]), name


@pytest.mark.parametrize("pid", [p for p, _ in R.variant_params()])
def test_softmax_trajectories_happen(pid):
    case = R.build((pid, TABLE[pid]))
    R.assert_trajectory(case)
    ref = R.reference(case)
    if case["variant"] == "identical":           # identical keys: the mean of the values
        n, npk, D = case["n_keys"], case["npad_k"], case["heads"] * 64
        V = case["vt"][:D * case["images"] * npk].reshape(D, case["images"], npk)[:, :, :n].astype(np.float64).mean(-1).T
        np.testing.assert_allclose(ref["ref"], np.broadcast_to(V[:, None, :], ref["ref"].shape), rtol=0, atol=1e-9)
    if case["variant"] == "shift_plus":          # the shift moves one query component and nothing of the result
        zero = R.build((pid.replace("shift_plus", "shift_zero"), TABLE[pid.replace("shift_plus", "shift_zero")]))
        np.testing.assert_array_equal(zero["k"], case["k"])
        np.testing.assert_array_equal(zero["vt"], case["vt"])
        d = case["q"] - zero["q"]
        nq, npq = case["n_queries"], case["npad_q"]
        real = np.concatenate([np.arange(i * npq, i * npq + nq) for i in range(case["images"])])
        assert (d[real][:, 63::64] == R.SHIFT).all() and np.count_nonzero(d[real]) == len(real) * case["heads"]
        np.testing.assert_allclose(R.reference(zero)["ref"], ref["ref"], rtol=0, atol=1e-9)
    if case["variant"] == "split_wave":          # without the rise the even queries are the same rows, the odd ones differ
        flat = R.make_case(**dict(TABLE[pid], rise=False))
        nq = case["n_queries"]
        np.testing.assert_array_equal(flat["q"][0:nq:2], case["q"][0:nq:2])
        assert not np.array_equal(flat["q"][1:nq:2], case["q"][1:nq:2])
        np.testing.assert_array_equal(flat["k"], case["k"])
        _, inf = R.emulate(flat, info=True)
        assert not inf["moved"][..., 1:].any()


@pytest.mark.parametrize("pid", [p for p, _ in R.bias_params() if p.rsplit("-", 1)[1] in R.BIAS_VARIANTS])
def test_biased_trajectories_happen(pid):
    case = R.build((pid, TABLE[pid]))
    R.assert_bias_trajectory(case, case["bias_kind"])
    if case["variant"]:
        R.assert_trajectory(case)


def test_targets_carry_weight_and_operands_are_what_the_module_says():
    for pid, kw in R.sweep_params() + R.bias_params():
        case = R.build((pid, kw))
        n, nq, npk, npq, images, D = kw["n_keys"], kw["n_queries"], kw["npad_k"], kw["npad_q"], kw["images"], kw["heads"] * 64
        for name in ("q", "k", "vt"):
            assert np.isfinite(case[name]).all() and np.array_equal(R.f16(case[name]), case[name]), (pid, name)
        assert case["q"].shape == (images * npq + R.SLACK, D) and case["k"].shape == (images * npk + R.SLACK, D)
        assert case["vt"].shape == (D * images * npk + R.SLACK,)
        K = case["k"][:images * npk].reshape(images, npk, D)
        vt = case["vt"][:D * images * npk].reshape(D, images, npk)
        if npk > n:
            assert np.abs(K[:, n:]).max() > 1.0 and (vt[:, :, n:] == R.PAD_V).all()
        assert (case["vt"][-R.SLACK:] == R.PAD_V).all() and np.abs(case["k"][-R.SLACK:]).max() > 1.0
        Q = case["q"][:images * npq].reshape(images, npq, D)
        assert (np.abs(Q[:, nq:]) == R.PAD_Q).all() and (np.abs(case["q"][-R.SLACK:]) == R.PAD_Q).all()
        if images > 1:
            assert not np.array_equal(K[0, :n], K[1, :n]) and not np.array_equal(Q[0, :nq], Q[1, :nq])
        if n >= 2 and kw["variant"] is None and kw["bias"] is None:
            p = R.reference(case, bounds=False)["p"]
            w = np.take_along_axis(p, case["targets"][..., None], -1)[..., 0]
            assert 0.2 <= np.median(w) <= 0.95, (pid, np.median(w))
        b = case["bias"]
        if b is not None:
            assert b["qcode"].shape == (images * npq + R.SLACK, 3) and b["kcode"].shape == (images * npk + R.SLACK, 4)
            for c in (b["qcode"], b["kcode"]):
                assert c[:, 0].min() >= 0 and c[:, 0].max() <= b["dp"] and c[:, 1:3].min() >= 0 and c[:, 1:3].max() <= b["dx"]
            valid = b["kcode"][:images * npk, 3].reshape(images, npk)
            assert (valid[:, n:] == 1).all() and (b["kcode"][images * npk:, 3] == 1).all(), "padding keys are not masked"
            masks = [tuple(valid[i, :n]) for i in range(images)]
            assert len(set(masks)) == images, "a different mask per image"


def test_derived_cases_of_the_isolation_checks():
    for pk in R.isolation_params():
        case = R.build(pk)
        ref = R.reference(case, bounds=False)["ref"]
        for i in range(case["images"]):
            np.testing.assert_array_equal(R.reference(R.take_image(case, i), bounds=False)["ref"][0], ref[i])
        for h in range(case["heads"]):
            np.testing.assert_allclose(R.reference(R.take_head(case, h), bounds=False)["ref"], ref[..., h * 64:h * 64 + 64], rtol=0, atol=1e-13)
        zero = R.zero_padding(case)
        np.testing.assert_array_equal(R.reference(zero, bounds=False)["ref"], ref)
        if case["heads"] <= 2:
            np.testing.assert_array_equal(R.emulate(zero), R.emulate(case))


def test_kernel_constants_restated():
    src = open(R.__file__.replace("oracle/attn_flash_ref.py", "marie_icr_amd/csrc/attn_flash.hip")).read()
    for text in ("AT_QB = 128, AT_KT = 64", "constexpr float RESCALE_AT = 8.f;", "const int key = 32 * (kt >> 1) + 8 * (i >> 2) + 4 * (kt & 1) + (i & 3);",
                 "const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);"):
        assert text in src, text
    common = open(R.__file__.replace("oracle/attn_flash_ref.py", "marie_icr_amd/csrc/common.h")).read()
    assert "constexpr int ATTN_SLACK_ROWS = 128;" in common and "constexpr float MHIP_ATTN_MASKED = -1024.f;" in common
    assert sorted(R.tile_key_order().tolist()) == list(range(64))


def test_block_remap_is_a_bijection_for_every_block_count():
    for nblk in range(1, 4097):
        bid = np.arange(nblk)
        q, r, xcd = nblk >> 3, nblk & 7, bid & 7
        L = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + (bid >> 3)
        assert np.array_equal(np.sort(L), bid), nblk
    for nblk in (1, 3, 7, 8, 9, 15, 17, 25, 4096):
        on_xcd = {}
        for b in range(nblk):
            on_xcd.setdefault(b & 7, []).append(R.xcd_remap(b, nblk))
        for ls in on_xcd.values():                 # consecutive logical blocks share an XCD
            assert ls == list(range(ls[0], ls[0] + len(ls)))


def test_case_table_covers_every_listed_edge():
    sweep = [kw for _, kw in R.sweep_params()]
    assert len(set(IDS)) == len(IDS)
    for layout in (R.FUSED, R.SPLIT):
        mine = [kw for kw in sweep if kw["layout"] == layout]
        assert {kw["n_keys"] for kw in mine} >= set(R.N_KEYS), layout
        assert {kw["heads"] for kw in mine} >= set(R.HEADS) and {kw["images"] for kw in mine} == {1, 2, 3}
        assert {kw["npad_k"] - R.ceil8(kw["n_keys"]) for kw in mine} >= {0, 8}
    assert {kw["n_queries"] for kw in sweep if kw["layout"] == R.SPLIT} >= set(R.N_QUERIES)
    assert {kw["n_queries"] for kw in sweep if kw["layout"] == R.FUSED} >= set(R.N_QUERIES)
    assert {kw["npad_q"] - R.ceil8(kw["n_queries"]) for kw in sweep if kw["layout"] == R.SPLIT} >= {0, 8}
    assert any(kw["layout"] == R.SPLIT and kw["npad_q"] != kw["npad_k"] and kw["n_queries"] != kw["n_keys"] for kw in sweep)
    assert any(kw["layout"] == R.FUSED and kw["n_queries"] < kw["n_keys"] for kw in sweep)
    far = [kw for kw in sweep if kw["n_queries"] == 100 and kw["npad_q"] == 264 and kw["layout"] == R.SPLIT]
    assert len(far) == 1 and far[0]["images"] >= 2
    assert {R.ntiles(kw["n_keys"]) for kw in sweep} >= {1, 2, 3, 4, 10}
    # no padding rows: the key behind the last one is the next image's row 0, or the slack
    assert any(kw["npad_k"] == kw["n_keys"] and kw["images"] >= 2 for kw in sweep)
    assert any(kw["npad_k"] == kw["n_keys"] and kw["n_keys"] % 64 == 0 for kw in sweep)
    blocks = {R.nqb(kw["n_queries"]) * kw["heads"] * kw["images"] for kw in sweep}
    assert blocks >= set(R.BLOCK_COUNTS), set(R.BLOCK_COUNTS) - blocks
    var = [kw for _, kw in R.variant_params()]
    assert [kw["variant"] for kw in var] == list(R.VARIANTS)
    assert all(kw["images"] >= 2 and kw["heads"] >= 2 and R.ntiles(kw["n_keys"]) >= 5 for kw in var)
    bias = R.bias_params()
    assert {kw["n_keys"] for _, kw in bias if kw["variant"] is None} == {65, 197, 264}
    assert {kw["images"] for _, kw in bias} == {2, 3}
    assert {(kw["bias"]["dp"], kw["bias"]["dx"]) for _, kw in bias} == {(7, 9), (511, 1000)}
    assert {p.rsplit("-", 1)[1] for p, _ in bias} >= set(R.BIAS_VARIANTS)
    assert {kw["layout"] for _, kw in bias} == {R.FUSED, R.SPLIT}
    assert all(kw["n_keys"] <= 577 and kw["n_queries"] <= 577 for _, kw in ALL + R.isolation_params())
    iso = [kw for _, kw in R.isolation_params()]
    assert all(kw["images"] >= 2 and kw["heads"] >= 2 for kw in iso) and any(kw["bias"] for kw in iso)
    assert {kw["layout"] for kw in iso} == {R.FUSED, R.SPLIT}
