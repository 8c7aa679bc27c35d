"""CPU checks of oracle/decode_attention_ref.py, the fp64 reference and operand sets of tests/test_decode_attention_gpu.py: the
reference is softmax attention, the ancestry tables follow the product's recurrence, and every likely indexing bug of a decode
attention kernel moves the reference of every case it applies to by at least ten times the GPU test's bar — so a kernel with
any of these bugs cannot pass that test."""
import numpy as np
import pytest

from oracle import decode_attention_ref as R


def test_reference_is_softmax_attention():
    rng = np.random.default_rng(0)
    q, K, V = rng.normal(size=(3, 128)), rng.normal(size=(3, 5, 128)), rng.normal(size=(3, 5, 128))
    got = R.attention(q, K, V, 2)
    for r in range(3):
        for h in range(2):
            sl = slice(64 * h, 64 * h + 64)
            s = K[r, :, sl] @ q[r, sl]
            p = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
            np.testing.assert_allclose(got[r, sl], p @ V[r, :, sl], rtol=1e-12, atol=1e-12)


def test_ancestry_follows_the_product_recurrence():
    """anc[r][s] is the slot the hypothesis in row r wrote at step s: its own row at the last step, and a prefix shared with the
    rows of its crop it descends from; never a slot of another crop"""
    rng = np.random.default_rng(1)
    crops, beam, n = 3, 3, 40
    anc = R.beam_ancestry(rng, crops, beam, n, n + 1)
    M = crops * beam
    assert (anc[:, n - 1] == np.arange(M)).all()
    assert (anc[:, :n] // beam == (np.arange(M) // beam)[:, None]).all()
    # a row's slot at step s was written by a row whose own history, up to s, is the prefix
    for r in range(M):
        for s in range(n - 1):
            assert anc[r, s] != anc[r, s + 1]          # a row never continues itself: the slot changes every step
    shared = sum(len({tuple(anc[r, :n // 2]) for r in range(c * beam, c * beam + beam)}) < beam for c in range(crops))
    assert shared >= 1, "rows of a crop should share prefixes"


@pytest.mark.parametrize("pid,kw", R.self_params(), ids=[p for p, _ in R.self_params()])
def test_each_kernel_bug_moves_the_self_attention_reference(pid, kw):
    case = R.self_case(**kw)
    ref = R.reference(case)
    assert np.isfinite(ref).all()
    bar = R.bars(kw["f16"], ref)[0]
    muts = R.mutations(case)
    want = {"swap_heads_0_1", "row0_ancestry_for_all"}
    if kw["n_keys"] >= 2:
        want |= {"drop_last_key", "drop_first_key", "anc_from_step_plus_1", "anc_from_step_minus_1"}
    assert set(muts) == want
    for name, m in muts.items():
        assert np.abs(m - ref).max() >= 10 * bar, (pid, name, np.abs(m - ref).max(), bar)


@pytest.mark.parametrize("pid,kw", R.cross_params(), ids=[p for p, _ in R.cross_params()])
def test_each_kernel_bug_moves_the_encoder_attention_reference(pid, kw):
    case = R.cross_case(**kw)
    ref = R.reference(case)
    assert np.isfinite(ref).all()                       # the NaN padding rows past n_keys are not part of the attention
    assert np.isnan(case["k"][:, kw["n_keys"]:]).all() and case["k"].shape[1] > kw["n_keys"]
    bar = R.bars(kw["f16"], ref)[0]
    muts = R.mutations(case)
    assert set(muts) == ({"swap_heads_0_1"} | ({"drop_last_key", "drop_first_key"} if kw["n_keys"] >= 2 else set()))
    for name, m in muts.items():
        assert np.abs(m - ref).max() >= 10 * bar, (pid, name, np.abs(m - ref).max(), bar)


def test_sweep_straddles_every_dispatch_threshold():
    for t in R.DISPATCH:
        assert t in R.SELF_N_KEYS and (t + 1 in R.SELF_N_KEYS or t == R.DISPATCH[-1])
    assert 577 in R.CROSS_N_KEYS and 640 in R.CROSS_N_KEYS
