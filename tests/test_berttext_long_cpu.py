"""The host side of BERT sentence embeddings past 128 tokens, without a GPU: the restatement tests/bert_text_ref.py against what
transformers.BertModel computed at 129, 257 and 512 tokens (tests/golden/bert_text_long.npz, written by
tests/make_bert_text_long_golden.py) — the pin that the streamed attention's GPU tests (tests/test_berttext_long_gpu.py) stand on
—, the batching plan with a routing boundary, the new export and the length limits of encode_texts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_long as RL  # noqa: E402
import bert_text_ref as R  # noqa: E402

SHORT_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_text.npz")


@pytest.fixture(scope="module")
def golden():
    return RL.load_long_golden()


@pytest.fixture(scope="module")
def emb_mod():
    import __graft_entry__ as g

    g.build()
    from marie_icr_amd import embeddings

    return embeddings


# ---------------------------------------------------------------------------------------------------- restatement vs transformers
@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_matches_transformers_bert_past_128_tokens(golden, name):
    g = golden[name]
    cfg = RL.CONFIGS[name]
    assert list(g["lens"]) == RL.LENS and g["ids"].shape == (3, RL.NPAD)
    assert g["hidden_rows"].dtype == np.float64 and g["hidden_rows"].shape == (cfg["depth"] + 1, 3, 4, cfg["dim"])
    assert np.array_equal(g["rows"], RL.stored_rows(RL.LENS))
    assert 0.5 <= np.abs(g["hidden_rows"]).max() <= 10
    taps, mean = R.forward(g["state"], cfg, g["ids"], g["lens"])
    _, mean_norm = R.forward(g["state"], cfg, g["ids"], g["lens"], "mean", True)
    _, cls = R.forward(g["state"], cfg, g["ids"], g["lens"], "cls")
    # the bars of tests/test_berttext_cpu.py for the short golden
    for what, got, want in (("hidden rows", RL.take_rows(taps, g["rows"]), g["hidden_rows"]), ("mean", mean, g["mean"]),
                            ("mean, normalised", mean_norm, g["mean_norm"]), ("cls", cls, g["cls"])):
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"config {name} {what}: max |d| / max |x| = {rel:.2e}")
        assert rel <= 1e-9
    assert np.allclose(np.sqrt((mean_norm ** 2).sum(-1)), 1.0, atol=1e-12)


def test_blocked_attention_reference_is_the_restatements():
    rng = np.random.default_rng(3)
    q, k, v = (rng.standard_normal((1, 72, 32)) for _ in range(3))
    for slopes in (None, np.array([0.25])):
        for f16 in (False, True):
            want = R.attention(q, k, v, [50], 1, slopes, f16)[0]
            got = RL.attention_blocked(q[0], k[0], v[0], 50, None if slopes is None else slopes[0], f16, step=16)
            assert np.abs(got - want).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------- batching plan
def _plan_before(lengths, max_group, rows_budget=None):
    """plan_text_groups as it was before it took `boundary`, word for word"""
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    groups = []
    at = 0
    while at < len(order):
        end = min(at + max_group, len(order))
        npad = (lengths[order[end - 1]] + 7) // 8 * 8
        # a shorter group of the same start never needs more rows a text
        while rows_budget is not None and end - at > 1 and (end - at) * npad > rows_budget:
            end -= 1
            npad = (lengths[order[end - 1]] + 7) // 8 * 8
        groups.append((npad, order[at:end]))
        at = end
    return groups


def test_plan_text_groups_with_a_boundary(emb_mod):
    rng = np.random.default_rng(5)
    lengths = [int(n) for n in rng.integers(3, 601, 200)] + [128, 129, 136, 128, 3, 600]
    for chunk, budget in ((1024, None), (7, None), (64, 2048), (1, None), (1024, 600), (16, 524288)):
        groups = emb_mod.plan_text_groups(lengths, chunk, budget, boundary=128)
        seen = [i for _, members in groups for i in members]
        assert sorted(seen) == list(range(len(lengths)))                       # every text once
        for npad, members in groups:
            own = [lengths[i] for i in members]
            assert max(own) <= 128 or min(own) > 128, "a group straddles the boundary"
            assert npad % 8 == 0 and npad - 8 < max(own) <= npad               # one npad: the longest rounded up to 8
            assert (npad <= 128) == (max(own) <= 128)
            assert len(members) <= chunk
            if budget is not None:
                assert len(members) * npad <= budget or len(members) == 1
        flat = [lengths[i] for i in seen]
        assert flat == sorted(flat)
        assert any(max(lengths[i] for i in mem) == 128 for _, mem in groups) and any(min(lengths[i] for i in mem) == 129 for _, mem in groups)
        # without the keyword: the plan as it was
        assert emb_mod.plan_text_groups(lengths, chunk, budget) == _plan_before(lengths, chunk, budget)
        assert emb_mod.plan_text_groups(lengths, chunk, budget, boundary=None) == _plan_before(lengths, chunk, budget)
    # nothing on the far side: the boundary changes nothing
    short = [n for n in lengths if n <= 128]
    assert emb_mod.plan_text_groups(short, 16, 512, boundary=128) == _plan_before(short, 16, 512)
    assert emb_mod.plan_text_groups([], 4, boundary=128) == []
    assert emb_mod.plan_text_groups([5, 130, 7, 128, 129], 8, boundary=128) == [(128, [0, 2, 3]), (136, [4, 1])]
    assert emb_mod.plan_text_groups([5, 130, 7, 128, 129], 8) == [(136, [0, 2, 3, 4, 1])]


# ---------------------------------------------------------------------------------------------------- the surface
def test_new_symbol_and_constants(emb_mod):
    from marie_icr_amd import _lib

    lib = _lib.load()
    assert "mhip_berttext_attention_long_host" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "mhip_berttext_attention_long_host")
    assert emb_mod.BERT_LONG_MAX_TOKENS == 8192 and emb_mod.BERT_MAX_TOKENS == 128
    assert callable(emb_mod.long_attention_host)
    # no profiler slot of its own
    names = [lib.mhip_kernel_name(k).decode() for k in range(lib.mhip_kernel_count())]
    assert names[-1] == "berttext_pool" and "attn_long" not in names


def test_encode_texts_limits_past_128(emb_mod):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    tok = WordPieceTokenizer(R.load_golden(SHORT_GOLDEN)[1]["vocab"])
    e = emb_mod.BertTextEmbeddings.__new__(emb_mod.BertTextEmbeddings)      # encode_texts needs the tokenizer and the limit alone
    e.tokenizer, e.max_tokens = tok, 512
    text = "the invoice total " * 200                                      # 600 pieces
    assert len(e.encode_texts(["the invoice total " * 170])[0]) == 512
    cut = e.encode_texts([text], truncation=True)[0]
    assert len(cut) == 512 and cut[0] == tok.cls_id and cut[-1] == tok.sep_id
    with pytest.raises(ValueError, match="too long: 602 tokens"):
        e.encode_texts(["the", text])
