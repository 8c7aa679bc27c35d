"""The host side of the BERT sentence encoders (marie_icr_amd/embeddings.py, wordpiece_tokenizer.py) without a GPU: the
restatement tests/bert_text_ref.py against what transformers.BertModel computed (tests/golden/bert_text.npz, written by
tests/make_bert_text_golden.py), the tokenizer against transformers.BertTokenizer, ALiBi slopes, the state loaders, the model
directory, the batching plan and the refusals."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_text.npz")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def emb_mod():
    import __graft_entry__ as g

    g.build()
    from marie_icr_amd import embeddings

    return embeddings


# ---------------------------------------------------------------------------------------------------- restatement vs transformers
@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_matches_transformers_bert(golden, name):
    g = golden[0][name]
    cfg = R.CONFIG_A if name == "A" else R.CONFIG_B
    assert g["hidden"].dtype == np.float64 and g["hidden"].shape == (cfg["depth"] + 1, 4, 24, cfg["dim"])
    assert 0.5 <= np.abs(g["hidden"]).max() <= 10
    taps, mean = R.forward(g["state"], cfg, g["ids"], g["lens"])
    _, mean_norm = R.forward(g["state"], cfg, g["ids"], g["lens"], "mean", True)
    _, cls = R.forward(g["state"], cfg, g["ids"], g["lens"], "cls")
    for what, got, want in (("hidden states", taps, g["hidden"]), ("mean", mean, g["mean"]), ("mean, normalised", mean_norm, g["mean_norm"]),
                            ("cls", cls, g["cls"])):
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"config {name} {what}: max |d| / max |x| = {rel:.2e}")
        assert rel <= 1e-9
    assert np.allclose(np.sqrt((mean_norm ** 2).sum(-1)), 1.0, atol=1e-12)


def test_f16_restatement_differs_by_roundings_only(golden):
    g = golden[0]["B"]
    taps, emb = R.forward(g["state"], R.CONFIG_B, g["ids"], g["lens"])
    taps16, emb16 = R.forward(g["state"], R.CONFIG_B, g["ids"], g["lens"], f16=True)
    m = R.valid_rows(g["lens"], g["ids"].shape[1])
    err = np.abs(taps16 - taps)[:, m].max()
    print(f"f16 restatement against float64: stream {err:.2e}, embeddings {np.abs(emb16 - emb).max():.2e}")
    assert np.array_equal(taps16[0], taps[0])      # nothing is rounded before the first GEMM
    assert 1e-5 < err < 5e-2


def test_restatement_variants_differ(golden):
    g = golden[0]["B"]
    sd = R.make_state(R.CONFIG_B_JINA, 3)
    ids, lens = g["ids"], g["lens"]
    taps, emb = R.forward(sd, R.CONFIG_B_JINA, ids, lens)
    assert 0.5 <= np.abs(taps).max() <= 10
    # no position table: two rows of one id are told apart by their ALiBi distances to the other ids alone
    same = np.array([[7, 7, 9, 9, 9, 9, 9, 9]], np.int32)
    t, _ = R.forward(sd, R.CONFIG_B_JINA, same, [8])
    assert np.array_equal(t[0][0, 0], t[0][0, 1]) and np.abs(t[-1][0, 0] - t[-1][0, 1]).max() > 1e-3
    # a padding row is never a key
    other = ids.copy()
    other[0, lens[0]:] = 9
    t2, e2 = R.forward(sd, R.CONFIG_B_JINA, other, lens)
    assert np.array_equal(e2, emb) and np.array_equal(t2[:, 0, :lens[0]], taps[:, 0, :lens[0]])


# ---------------------------------------------------------------------------------------------------- tokenizer
@pytest.mark.parametrize("mode", ["uncased", "cased"])
def test_tokenizer_matches_the_golden_tokenisations(golden, mode):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    tk = golden[1]
    tok = WordPieceTokenizer(tk["vocab"], do_lower_case=mode == "uncased")
    assert len(tk["texts"]) >= 30 and 70 <= len(tk["vocab"]) <= 90
    for again in range(2):      # the second round finds the ids of the ASCII words remembered
        for text, want in zip(tk["texts"], tk["ids"][mode]):
            assert tok.encode(text) == want, repr(text)
            assert tok.piece_ids(text) == [tok.vocab[p] for p in tok.tokenize(text)]
    assert "invoice" in tok._word_ids and not any(w for w in tok._word_ids if not w.isascii())
    flat = [i for ids in tk["ids"][mode] for i in ids]
    assert flat.count(tok.unk_id) >= 5 and len(set(flat)) > 40      # the cases reach unknown pieces and most of the vocabulary


@pytest.mark.parametrize("lower", [True, False])
def test_tokenizer_matches_transformers(golden, lower):
    transformers = pytest.importorskip("transformers")
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    tk = golden[1]
    ref = transformers.BertTokenizer(vocab={v: i for i, v in enumerate(tk["vocab"])}, do_lower_case=lower)
    tok = WordPieceTokenizer(tk["vocab"], do_lower_case=lower)
    extra = ["Total due: $50 (net)", "ÀÉÎÕÜ àéîõü", "a-b_c+1=2", "中文日本", "the  \t invoice\n", "x" * 100 + "y", "naïve café", "I’m “the” total…"]
    for text in tk["texts"] + extra:
        assert tok.encode(text) == ref(text)["input_ids"], repr(text)


def test_tokenizer_truncation_and_padding(golden, tmp_path):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    tk = golden[1]
    with open(tmp_path / "vocab.txt", "w", encoding="utf-8") as f:
        f.write("\n".join(tk["vocab"]) + "\n")
    tok = WordPieceTokenizer.from_dir(str(tmp_path))
    assert tok.do_lower_case and len(tok) == len(tk["vocab"])
    with open(tmp_path / "tokenizer_config.json", "w") as f:
        json.dump({"do_lower_case": False}, f)
    assert not WordPieceTokenizer.from_dir(str(tmp_path)).do_lower_case
    assert WordPieceTokenizer.from_dir(str(tmp_path / "nowhere")) is None
    long = " ".join(["the invoice total"] * 20)
    full = tok.encode(long)
    assert len(full) == 62 and full[0] == tok.cls_id and full[-1] == tok.sep_id
    cut = tok.encode(long, 10)
    assert cut == [tok.cls_id] + full[1:9] + [tok.sep_id]
    assert tok.encode("the", 10) == tok.encode("the")
    ids, lens = tok.pad([tok.encode("the"), cut], 16)
    assert ids.shape == (2, 16) and ids.dtype == np.int32 and list(lens) == [3, 10]
    assert (ids[0, 3:] == tok.pad_id).all() and list(ids[1, :10]) == cut
    with pytest.raises(ValueError):
        tok.pad([full], 8)


# ---------------------------------------------------------------------------------------------------- ALiBi slopes
def test_alibi_slopes_closed_forms(emb_mod):
    want8 = np.array([2.0 ** -(i + 1) for i in range(8)])
    want12 = np.array([2.0 ** -(i + 1) for i in range(8)] + [2.0 ** -0.5, 2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5])
    for heads, want in ((8, want8), (12, want12)):
        np.testing.assert_allclose(emb_mod.alibi_slopes(heads), want, rtol=1e-7)
        np.testing.assert_allclose(R.alibi_slopes(heads), want, rtol=1e-15)
    np.testing.assert_allclose(emb_mod.alibi_slopes(2), [2.0 ** -4, 2.0 ** -8], rtol=1e-7)
    np.testing.assert_allclose(emb_mod.alibi_slopes(3), [2.0 ** -4, 2.0 ** -8, 2.0 ** -2], rtol=1e-7)
    with pytest.raises(emb_mod.MarieHipError):
        emb_mod.alibi_slopes(0)


# ---------------------------------------------------------------------------------------------------- state loaders
def test_load_bert_text_state_both_schemes(emb_mod):
    sd = R.make_state(R.CONFIG_A, 1)
    state, cfg = emb_mod.load_bert_text_state(sd, R.config_json(R.CONFIG_A))
    assert (cfg.vocab, cfg.max_position, cfg.type_vocab, cfg.dim, cfg.heads, cfg.depth, cfg.ffn) == (80, 128, 2, 64, 2, 2, 256)
    assert (cfg.position, cfg.mlp, cfg.pool, cfg.normalize) == (emb_mod.POS_ABSOLUTE, emb_mod.MLP_GELU, emb_mod.POOL_MEAN, 0)
    assert abs(cfg.ln_eps - 1e-12) < 1e-18
    assert set(state) == set(sd) and all(v.dtype == np.float32 for v in state.values())
    # a "bert." prefix, a pooler and position_ids do not matter; torch tensors are taken
    import torch

    dressed = {"bert." + k: torch.from_numpy(v) for k, v in sd.items()}
    dressed["bert.pooler.dense.weight"] = torch.zeros(64, 64)
    dressed["bert.embeddings.position_ids"] = torch.arange(128)[None]
    state2, _ = emb_mod.load_bert_text_state(dressed, R.config_json(R.CONFIG_A))
    assert set(state2) == set(sd) and all(np.array_equal(state2[k], sd[k]) for k in sd)
    # JinaBERT: from the config, and from the keys alone
    jd = R.make_state(R.CONFIG_B_JINA, 2)
    for conf in (R.config_json(R.CONFIG_B_JINA),
                 {k: v for k, v in R.config_json(R.CONFIG_B_JINA).items() if k not in ("feed_forward_type", "position_embedding_type")}):
        jstate, jcfg = emb_mod.load_bert_text_state(jd, conf)
        assert (jcfg.position, jcfg.mlp, jcfg.dim) == (emb_mod.POS_ALIBI, emb_mod.MLP_GEGLU, 128)
        assert jstate["encoder.layer.1.mlp.gated_layers.weight"].shape == (512, 128)
        assert not any("position_embeddings" in k or "intermediate" in k for k in jstate)


def test_load_bert_text_state_names_what_is_wrong(emb_mod):
    sd = R.make_state(R.CONFIG_A, 1)
    conf = R.config_json(R.CONFIG_A)
    for key in ("encoder.layer.1.output.dense.bias", "embeddings.LayerNorm.weight", "embeddings.position_embeddings.weight"):
        with pytest.raises(emb_mod.MarieHipError, match=key.replace(".", r"\.")):
            emb_mod.load_bert_text_state({k: v for k, v in sd.items() if k != key}, conf)
    bad = dict(sd, **{"encoder.layer.0.intermediate.dense.weight": np.zeros((128, 64), np.float32)})
    with pytest.raises(emb_mod.MarieHipError, match=r"encoder\.layer\.0\.intermediate\.dense\.weight.*\(128, 64\)"):
        emb_mod.load_bert_text_state(bad, conf)
    with pytest.raises(emb_mod.MarieHipError, match="mlp.gated_layers"):      # a BERT checkpoint under a JinaBERT config
        emb_mod.load_bert_text_state(sd, dict(conf, feed_forward_type="geglu"))
    with pytest.raises(emb_mod.MarieHipError, match="hidden_size"):
        emb_mod.load_bert_text_state(sd, {k: v for k, v in conf.items() if k != "hidden_size"})
    with pytest.raises(NotImplementedError, match="relative_key"):
        emb_mod.load_bert_text_state(sd, dict(conf, position_embedding_type="relative_key"))
    with pytest.raises(emb_mod.MarieHipError):
        emb_mod.load_bert_text_state({}, conf)


# ---------------------------------------------------------------------------------------------------- model directory
def test_model_directory_parsing(emb_mod, tmp_path):
    d = str(tmp_path)
    assert emb_mod.read_sentence_model_dir(d) == {}
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
                   {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}], f)
    os.mkdir(os.path.join(d, "1_Pooling"))
    pooling = {"word_embedding_dimension": 384, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
               "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump(pooling, f)
    with open(os.path.join(d, "sentence_bert_config.json"), "w") as f:
        json.dump({"max_seq_length": 256, "do_lower_case": False}, f)
    assert emb_mod.read_sentence_model_dir(d) == {"pooling": "mean", "normalize": True, "max_seq_length": 256}
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump(dict(pooling, pooling_mode_cls_token=True, pooling_mode_mean_tokens=False), f)
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump([{"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}], f)
    assert emb_mod.read_sentence_model_dir(d) == {"pooling": "cls", "normalize": False, "max_seq_length": 256}
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump(dict(pooling, pooling_mode_max_tokens=True, pooling_mode_mean_tokens=False), f)
    with pytest.raises(NotImplementedError, match="max_tokens"):
        emb_mod.read_sentence_model_dir(d)


def test_class_defaults(emb_mod):
    st, jina = emb_mod.SentenceTransformerEmbeddings, emb_mod.JinaEmbeddings
    assert (st.POOLING, st.NORMALIZE, st.MAX_LENGTH, st.TOTAL_TOKENS_IS_WIDTH) == ("mean", True, 256, True)
    assert (jina.POOLING, jina.NORMALIZE, jina.MAX_LENGTH, jina.TOTAL_TOKENS_IS_WIDTH) == ("mean", False, None, False)
    assert issubclass(st, emb_mod.EmbeddingsBase) and issubclass(jina, emb_mod.BertTextEmbeddings)
    assert emb_mod.BERT_MAX_TOKENS == 128


# ---------------------------------------------------------------------------------------------------- batching plan
def test_plan_text_groups(emb_mod):
    rng = np.random.default_rng(5)
    lengths = [int(n) for n in rng.integers(3, 129, 200)] + [128, 3, 8, 9, 16, 17]
    for chunk, budget in ((1024, None), (7, None), (64, 512), (1, None), (1024, 128)):
        groups = emb_mod.plan_text_groups(lengths, chunk, budget)
        seen = [i for _, members in groups for i in members]
        assert sorted(seen) == list(range(len(lengths)))                       # every text once
        for npad, members in groups:
            longest = max(lengths[i] for i in members)
            assert npad % 8 == 0 and npad <= 128 and npad - 8 < longest <= npad      # one npad: the longest rounded up to 8
            assert len(members) <= chunk
            if budget is not None:
                assert len(members) * npad <= budget or len(members) == 1
        flat = [lengths[i] for i in seen]
        assert flat == sorted(flat)                                            # sorted by token count
        out = np.empty(len(lengths), np.int64)                                 # what embed_texts does with the plan
        for _, members in groups:
            out[members] = [lengths[i] for i in members]
        assert list(out) == lengths                                            # rows land in input order
    assert emb_mod.plan_text_groups([], 4) == []
    assert emb_mod.plan_text_groups([5, 30, 7], 8) == [(32, [0, 2, 1])]


# ---------------------------------------------------------------------------------------------------- refusals without a device
def test_refusals_before_any_device_work(emb_mod, golden):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    tok = WordPieceTokenizer(golden[1]["vocab"])
    sd, conf = R.make_state(R.CONFIG_A, 1), R.config_json(R.CONFIG_A)
    for cls in (emb_mod.SentenceTransformerEmbeddings, emb_mod.JinaEmbeddings):
        with pytest.raises(emb_mod.MarieHipError, match="use_gpu=False"):
            cls(state=sd, config=conf, tokenizer=tok, use_gpu=False)
        with pytest.raises(emb_mod.MarieHipError, match="model directory"):
            cls()
    with pytest.raises(emb_mod.MarieHipError, match="word table"):
        emb_mod.JinaEmbeddings(state=sd, config=conf, tokenizer=WordPieceTokenizer(golden[1]["vocab"] + [f"w{i}" for i in range(10)]))
    # the 128-token limit: encode_texts needs the tokenizer and the limit alone
    e = emb_mod.BertTextEmbeddings.__new__(emb_mod.BertTextEmbeddings)
    e.tokenizer, e.max_tokens = tok, emb_mod.BERT_MAX_TOKENS
    assert len(e.encode_texts(["the invoice total " * 42])[0]) == 128
    with pytest.raises(ValueError, match="too long: 131 tokens"):
        e.encode_texts(["the", "the invoice total " * 43])
    cut = e.encode_texts(["the invoice total " * 43], truncation=True)[0]
    assert len(cut) == 128 and cut[0] == tok.cls_id and cut[-1] == tok.sep_id


def test_abi_symbols_present(emb_mod):
    from marie_icr_amd import _lib

    lib = _lib.load()
    for name in ("create", "destroy", "set_tensor", "finalize", "alloc_arena", "arena", "workspace_bytes", "embed_host", "embed_pairs_host",
                 "debug_taps_host", "embed_rows_host", "attention_host", "geglu_host", "pool_host", "alibi_slopes"):
        assert f"mhip_berttext_{name}" in _lib.EXPORTED_SYMBOLS and hasattr(lib, f"mhip_berttext_{name}")
    names = [lib.mhip_kernel_name(k).decode() for k in range(lib.mhip_kernel_count())]
    assert names[31:] == ["lev_ngrams", "attn_short", "berttext_embed", "geglu", "berttext_pool"]
    fields = [f for f, _ in _lib.BertTextConfig._fields_]
    assert fields == ["vocab", "max_position", "type_vocab", "dim", "heads", "depth", "ffn", "ln_eps", "position", "mlp", "pool", "normalize"]
