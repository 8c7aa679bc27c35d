"""The MPNet, RoBERTa and DistilBERT sentence encoders without a GPU: the restatement tests/sentence_families_ref.py against what
transformers computed (tests/golden/sentence_families.npz, written by tests/make_sentence_families_golden.py), the folded bias
table of mhip_berttext_rel_table against MPNetEncoder.relative_position_bucket, the loader, and the tokenizers against
MPNetTokenizer, RobertaTokenizer and DistilBertTokenizer."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402
import sentence_families_ref as S  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


@pytest.fixture(scope="module")
def emb_mod():
    import __graft_entry__ as g

    g.build()
    from marie_icr_amd import embeddings

    return embeddings


# ---------------------------------------------------------------------------------------------------- restatement vs transformers
@pytest.mark.parametrize("name", list(S.MODELS) + ["mpnet_b_long"])
def test_restatement_matches_transformers(golden, name):
    models, buckets, _ = golden
    g = models[name]
    cfg = S.MODELS["mpnet_b" if name == "mpnet_b_long" else name]
    assert g["hidden_rows"].dtype == np.float64 and g["hidden_rows"].shape == (cfg["depth"] + 1, len(g["lens"]), 4, cfg["dim"])
    assert 0.5 <= np.abs(g["hidden_rows"]).max() <= 10
    taps, mean = S.forward(g["state"], cfg, g["ids"], g["lens"], buckets)
    _, mean_norm = S.forward(g["state"], cfg, g["ids"], g["lens"], buckets, "mean", True)
    _, cls = S.forward(g["state"], cfg, g["ids"], g["lens"], buckets, "cls")
    for what, got, want in (("hidden rows", S.take_rows(taps, g["rows"]), g["hidden_rows"]), ("mean", mean, g["mean"]),
                            ("mean, normalised", mean_norm, g["mean_norm"]), ("cls", cls, g["cls"])):
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name} {what}: max |d| / max |x| = {rel:.2e}")
        assert rel <= 1e-9


def test_f16_restatement_differs_by_roundings_only(golden):
    models, buckets, _ = golden
    g, cfg = models["mpnet_b"], S.MODELS["mpnet_b"]
    taps, emb = S.forward(g["state"], cfg, g["ids"], g["lens"], buckets)
    taps16, emb16 = S.forward(g["state"], cfg, g["ids"], g["lens"], buckets, f16=True)
    valid = R.valid_rows(g["lens"], g["ids"].shape[1])
    assert np.array_equal(taps16[0], taps[0])
    assert 1e-5 < np.abs(taps16 - taps)[:, valid].max() < 0.05 and 1e-6 < np.abs(emb16 - emb).max() < 0.02


def test_the_bias_and_the_offset_matter(golden):
    """the restatement without the table, or with the position rows from 0, is far from the golden: the 1e-9 above pins both"""
    models, buckets, _ = golden
    g, cfg = models["mpnet_b"], S.MODELS["mpnet_b"]
    flat = dict(g["state"], **{"encoder.relative_attention_bias.weight": np.zeros((32, 2), np.float32)})
    assert np.abs(S.forward(flat, cfg, g["ids"], g["lens"], buckets)[1] - g["mean"]).max() > 1e-2
    assert np.abs(S.forward(g["state"], dict(cfg, pos_offset=0), g["ids"], g["lens"], buckets)[1] - g["mean"]).max() > 1e-2
    # the clamp is exercised by the long batch: its queries see keys 256 rows away on both sides
    long = models["mpnet_b_long"]
    assert long["ids"].shape == (3, 264) and list(long["lens"]) == [129, 131, 257]


# ---------------------------------------------------------------------------------------------------- the folded table
def test_rel_table_equals_the_library_bucket_for_every_distance(emb_mod, golden):
    _, buckets, _ = golden
    assert buckets.shape == (1201,)
    # keys before the query take buckets 0 .. 15, keys after it 16 .. 31; constant from 128 on each side
    at = lambda rel: int(buckets[rel + S.BUCKET_SPAN])      # noqa: E731
    assert (at(-16), at(-8), at(1), at(8), at(0)) == (10, 8, 17, 24, 0)
    assert set(buckets[:S.BUCKET_SPAN - 127]) == {15} and set(buckets[S.BUCKET_SPAN + 128:]) == {31}
    # weight[b][h] = b + 100 h reads the bucket back, exactly
    weight = (np.arange(32)[:, None] + 100.0 * np.arange(3)[None, :]).astype(np.float32)
    table = emb_mod.rel_table(32, 128, weight)
    assert table.shape == (3, 257) and table.dtype == np.float32
    d = np.arange(-600, 601)                                       # d = query - key, the bucket is of key - query
    got = table[:, np.clip(d, -128, 128) + 128]
    want = buckets[-d + S.BUCKET_SPAN][None, :] + 100.0 * np.arange(3)[:, None]
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(table, S.rel_table(weight, buckets).astype(np.float32))
    transformers = pytest.importorskip("transformers")
    import torch

    lib = transformers.models.mpnet.modeling_mpnet.MPNetEncoder.relative_position_bucket(torch.from_numpy(-d), 32, 128).numpy()
    assert np.array_equal(got[0], lib.astype(np.float32))


def test_rel_table_refuses_buckets_that_do_not_saturate(emb_mod):
    # 1024 buckets: distances below 256 have a bucket each, so the bucket still changes past 128
    with pytest.raises(emb_mod.MarieHipError, match="constant past the distance"):
        emb_mod.rel_table(1024, 128, np.zeros((1024, 2), np.float32))
    with pytest.raises(emb_mod.MarieHipError):
        emb_mod.rel_table(32, 8, np.zeros((32, 2), np.float32))      # max_distance = buckets / 4: the rule's logarithm of 1
    assert emb_mod.rel_table(32, 64, np.zeros((32, 2), np.float32)).shape == (2, 129)


# ---------------------------------------------------------------------------------------------------- the loader
@pytest.mark.parametrize("name,fields", [("mpnet_a", (2, 0, 32)), ("roberta", (2, 1, 0)), ("distilbert", (0, 0, 0))])
def test_load_sentence_encoder_state_per_family(emb_mod, name, fields):
    import torch

    cfg = S.MODELS[name]
    family = cfg["family"]
    sd, conf = S.make_state(cfg, 1), S.config_json(cfg)
    state, c, got_family = emb_mod.load_sentence_encoder_state(sd, conf)
    assert got_family == family and (c.pos_offset, c.type_vocab, c.rel_buckets) == fields
    assert c.rel_max_distance == (128 if family == "mpnet" else 0)
    assert (c.vocab, c.max_position, c.dim, c.heads, c.depth, c.ffn) == tuple(cfg[k] for k in ("vocab", "max_position", "dim", "heads", "depth", "ffn"))
    assert (c.position, c.mlp, c.pool, c.normalize) == (emb_mod.POS_ABSOLUTE, emb_mod.MLP_GELU, emb_mod.POOL_MEAN, 0)
    assert abs(c.ln_eps - cfg["eps"]) < 1e-12
    # every source tensor arrives once, under the canonical name, unchanged
    want = S.canonical(sd, family)
    assert set(state) == set(want) and all(np.array_equal(state[k], want[k]) and state[k].dtype == np.float32 for k in want)
    assert all(k.startswith("embeddings.") or k.startswith("encoder.") for k in state)
    # the family's prefix, a pooler and torch tensors; and the family from the keys alone
    dressed = {f"{family}.{k}": torch.from_numpy(v) for k, v in sd.items()}
    dressed[f"{family}.pooler.dense.weight"] = torch.zeros(cfg["dim"], cfg["dim"])
    state2, _, _ = emb_mod.load_sentence_encoder_state(dressed, conf)
    assert set(state2) == set(want) and all(np.array_equal(state2[k], want[k]) for k in want)
    bare = {k: v for k, v in conf.items() if k != "model_type"}
    assert emb_mod.load_sentence_encoder_state(dressed, bare)[2] == family
    # a missing or misshapen tensor is named by the family's own key
    lost = S.own_key(family, "encoder.layer.1.attention.self.key.weight")
    with pytest.raises(emb_mod.MarieHipError, match=lost.replace(".", r"\.")):
        emb_mod.load_sentence_encoder_state({k: v for k, v in sd.items() if k != lost}, conf)
    with pytest.raises(emb_mod.MarieHipError, match=lost.replace(".", r"\.") + " has shape"):
        emb_mod.load_sentence_encoder_state(dict(sd, **{lost: sd[lost][:, :8]}), conf)


def test_distilbert_eps_and_unknown_families(emb_mod):
    cfg = S.MODELS["distilbert"]
    sd = S.make_state(cfg, 1)
    _, c, _ = emb_mod.load_sentence_encoder_state(sd, dict(S.config_json(cfg), layer_norm_eps=1e-5))
    assert abs(c.ln_eps - 1e-12) < 1e-18                           # DistilBERT's LayerNorms are built with 1e-12
    # a field config.json leaves out takes the library's default (RobertaConfig: 1e-12, two token types, 512 positions)
    rcfg = dict(S.MODELS["roberta"], type_vocab=2, max_position=512)
    bare = {k: v for k, v in S.config_json(rcfg).items() if k not in ("layer_norm_eps", "type_vocab_size", "max_position_embeddings")}
    _, c, _ = emb_mod.load_sentence_encoder_state(S.make_state(rcfg, 2), bare)
    assert abs(c.ln_eps - 1e-12) < 1e-18 and (c.type_vocab, c.max_position, c.pos_offset) == (2, 512, 2)
    for kind in ("xlm-roberta", "albert", "deberta-v2", "t5"):
        with pytest.raises(NotImplementedError, match=kind):
            emb_mod.load_sentence_encoder_state(sd, dict(S.config_json(cfg), model_type=kind))
    with pytest.raises(emb_mod.MarieHipError, match="no n_heads"):
        emb_mod.load_sentence_encoder_state(sd, {k: v for k, v in S.config_json(cfg).items() if k != "n_heads"})
    no_bias = {k: v for k, v in S.make_state(S.MODELS["mpnet_a"], 1).items() if "relative_attention_bias" not in k}
    with pytest.raises(emb_mod.MarieHipError, match=r"encoder\.relative_attention_bias\.weight"):
        emb_mod.load_sentence_encoder_state(no_bias, S.config_json(S.MODELS["mpnet_a"]))


def test_a_bert_checkpoint_loads_as_before(emb_mod):
    sd = R.make_state(R.CONFIG_A, 1)
    for conf in (R.config_json(R.CONFIG_A), dict(R.config_json(R.CONFIG_A), model_type="bert")):
        state, cfg, family = emb_mod.load_sentence_encoder_state(sd, conf)
        old_state, old = emb_mod.load_bert_text_state(sd, conf)
        assert family == "bert" and list(state) == list(old_state) and all(np.array_equal(state[k], old_state[k]) for k in state)
        assert (cfg.vocab, cfg.max_position, cfg.type_vocab, cfg.dim, cfg.heads, cfg.depth, cfg.ffn) == (80, 128, 2, 64, 2, 2, 256)
        assert (cfg.position, cfg.mlp, cfg.pool, cfg.normalize) == (emb_mod.POS_ABSOLUTE, emb_mod.MLP_GELU, emb_mod.POOL_MEAN, 0)
        assert abs(cfg.ln_eps - 1e-12) < 1e-18 and (cfg.pos_offset, cfg.rel_buckets, cfg.rel_max_distance) == (0, 0, 0)
        assert all(getattr(cfg, f) == getattr(old, f) for f, _ in type(old)._fields_)
    jd = R.make_state(R.CONFIG_B_JINA, 2)
    _, jcfg, family = emb_mod.load_sentence_encoder_state(jd, R.config_json(R.CONFIG_B_JINA))
    assert family == "bert" and (jcfg.position, jcfg.mlp) == (emb_mod.POS_ALIBI, emb_mod.MLP_GEGLU)
    with pytest.raises(emb_mod.MarieHipError, match="Hugging Face BERT keys"):      # the old message, through the new loader
        emb_mod.load_sentence_encoder_state({k: v for k, v in sd.items() if "token_type" not in k}, R.config_json(R.CONFIG_A))


# ---------------------------------------------------------------------------------------------------- tokenizers
@pytest.mark.parametrize("case", ["mpnet_uncased", "mpnet_cased", "distilbert_uncased", "distilbert_cased"])
def test_wordpiece_matches_the_family_tokenizers(golden, case):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    family, mode = case.split("_")
    if family == "mpnet":
        tok = WordPieceTokenizer(S.MPNET_VOCAB, do_lower_case=mode == "uncased", cls_token="<s>", sep_token="</s>", pad_token="<pad>",
                                 unk_token="[UNK]", mask_token="<mask>")
        assert (tok.cls_id, tok.pad_id, tok.sep_id, tok.unk_id) == (0, 1, 2, 3)
    else:
        tok = WordPieceTokenizer(S.BERT_VOCAB, do_lower_case=mode == "uncased")
    want = golden[2][case]
    assert len(want) == len(S.WORDPIECE_TEXTS)
    for text, ids in zip(S.WORDPIECE_TEXTS, want):
        assert tok.encode(text) == ids, repr(text)
    assert sum(ids.count(tok.unk_id) for ids in want) >= 3 and max(len(ids) for ids in want) >= 10


def _bpe(tmp_path):
    from marie_icr_amd.document_classifier import ByteLevelBPE

    return ByteLevelBPE(*S.write_bpe_files(str(tmp_path)))


def test_byte_level_bpe_matches_roberta_on_whole_texts(golden, tmp_path):
    tok = _bpe(tmp_path)
    assert len(tok) == 5 + 256 + len(S.BPE_MERGES) and (tok.bos_id, tok.pad_id, tok.eos_id) == (0, 1, 2)
    want = golden[2]["roberta"]
    assert len(want) == len(S.BPE_TEXTS)
    for text, ids in zip(S.BPE_TEXTS, want):
        assert tok.encode(text) == ids, repr(text)
    assert tok.encode("") == [0, 2] and tok.unk_id not in [i for ids in want for i in ids]
    # no prefix space: the first word of a text and the same word after a blank are different tokens
    assert tok.encode("the the")[1:3] != tok.encode(" the the")[1:3]
    # the word-level entry the LayoutLMv3 path uses is untouched by the text cache
    assert tok.encode_word("the") == tok.encode(" the")[1:-1]
    fresh = _bpe(tmp_path)
    want = fresh.encode_word("\0the")
    assert tok.encode("\0the") and tok.encode_word("\0the") == want and tok.encode_word("the") == fresh.encode_word("the")


def test_tokenizers_from_a_model_directory(emb_mod, golden, tmp_path):
    from marie_icr_amd.document_classifier import ByteLevelBPE
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    d = str(tmp_path)
    with pytest.raises(emb_mod.MarieHipError, match=r"vocab\.txt.*vocab\.json and merges\.txt"):
        emb_mod.sentence_tokenizer_from_dir(d, "roberta")
    for only in ("tokenizer.json", "sentencepiece.bpe.model"):
        open(os.path.join(d, only), "w").close()
    with pytest.raises(emb_mod.MarieHipError, match=r"only tokenizer\.json, sentencepiece\.bpe\.model"):
        emb_mod.sentence_tokenizer_from_dir(d, "mpnet")
    S.write_bpe_files(d)
    tok = emb_mod.sentence_tokenizer_from_dir(d, "roberta")
    assert isinstance(tok, ByteLevelBPE) and tok.encode("the invoice total") == golden[2]["roberta"][0]
    with open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(S.MPNET_VOCAB) + "\n")
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump({"do_lower_case": False}, f)
    tok = emb_mod.sentence_tokenizer_from_dir(d, "mpnet")
    assert isinstance(tok, WordPieceTokenizer) and not tok.do_lower_case and (tok.cls_id, tok.pad_id, tok.sep_id) == (0, 1, 2)
    assert [tok.encode(t) for t in S.WORDPIECE_TEXTS] == golden[2]["mpnet_cased"]


def test_truncation_and_padding_with_the_family_pad(tmp_path):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    wp = WordPieceTokenizer(S.MPNET_VOCAB, cls_token="<s>", sep_token="</s>", pad_token="<pad>", mask_token="<mask>")
    for tok, text, first, last in ((wp, "the invoice total " * 10, 0, 2), (_bpe(tmp_path), "the invoice total" * 10, 0, 2)):
        full = tok.encode(text)
        cut = tok.encode(text, 12)
        assert len(full) > 12 and len(cut) == 12 and cut[0] == first and cut[-1] == last and cut[1:-1] == full[1:11]
        ids, lens = tok.pad([cut, full[:5]], 16)
        assert ids.dtype == np.int32 and ids.shape == (2, 16) and list(lens) == [12, 5]
        assert (ids[0, 12:] == 1).all() and (ids[1, 5:] == 1).all() and tok.pad_id == 1
        with pytest.raises(ValueError):
            tok.pad([full], 8)
        with pytest.raises(ValueError):
            tok.encode(text, 1)


# ---------------------------------------------------------------------------------------------------- the surface
def test_class_limits_and_refusals_before_any_device_work(emb_mod, tmp_path):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    cfg = S.MODELS["mpnet_a"]
    sd, conf = S.make_state(cfg, 1), S.config_json(cfg)
    big = WordPieceTokenizer(S.MPNET_VOCAB + [f"w{i}" for i in range(10)], cls_token="<s>", sep_token="</s>", pad_token="<pad>", mask_token="<mask>")
    with pytest.raises(emb_mod.MarieHipError, match="word table"):
        emb_mod.SentenceTransformerEmbeddings(state=sd, config=conf, tokenizer=big)
    with pytest.raises(NotImplementedError, match="xlm-roberta"):
        emb_mod.SentenceTransformerEmbeddings(state=sd, config=dict(conf, model_type="xlm-roberta"), tokenizer=big)
    # a directory without a vocabulary this build reads: refused with the files named, after the checkpoint was understood
    from safetensors.numpy import save_file

    d = str(tmp_path)
    save_file({"mpnet." + k: v for k, v in sd.items()}, os.path.join(d, "model.safetensors"))
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(conf, f)
    open(os.path.join(d, "tokenizer.json"), "w").close()
    with pytest.raises(emb_mod.MarieHipError, match=r"only tokenizer\.json"):
        emb_mod.SentenceTransformerEmbeddings(d)


def test_abi_and_kernel_names(emb_mod):
    from marie_icr_amd import _lib

    lib = _lib.load()
    for name in ("create_ex", "rel_table", "attention_rel_host", "attention_rel_long_host", "embed_rows_ex_host"):
        assert f"mhip_berttext_{name}" in _lib.EXPORTED_SYMBOLS and hasattr(lib, f"mhip_berttext_{name}")
    names = [lib.mhip_kernel_name(k).decode() for k in range(lib.mhip_kernel_count())]
    assert names[31:] == ["lev_ngrams", "attn_short", "berttext_embed", "geglu", "berttext_pool"]      # no new profiler slots
    assert [f for f, _ in _lib.SentenceEncoderConfig._fields_] == ["pos_offset", "rel_buckets", "rel_max_distance"]
    import ctypes

    assert ctypes.sizeof(_lib.SentenceEncoderConfig) == ctypes.sizeof(_lib.BertTextConfig) + 12
    assert _lib.SentenceEncoderConfig.pos_offset.offset == ctypes.sizeof(_lib.BertTextConfig)
