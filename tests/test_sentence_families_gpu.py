"""MPNet, RoBERTa and DistilBERT sentence encoders on the MI355X: the relative-distance table as a third score term of attn_short and
attn_long (marie_icr_amd/csrc/attn_seq.hip) alone, the embedding kernel with a position offset and no type row, the encoders
against tests/sentence_families_ref.py — the float64 restatement that tests/test_sentence_families_cpu.py pins to transformers
through tests/golden/sentence_families.npz — and the public classes.

Bars, those of tests/test_berttext_gpu.py and tests/test_berttext_long_gpu.py:
  * fp32: 1e-3 absolute on O(1) quantities for the kernels, stream taps and embeddings, 1e-5 for cosines;
  * f16: E_ref = max |f16-rounded restatement - float64 restatement| is computed here on the CPU for each case, and
    max |kernel - float64 restatement| <= 2 E_ref;
  * a text's rows do not depend on npad, on its batch or on what lies past its length: bitwise, in both precisions.
Every test prints its figures before it asserts.

First MI355X run: recorded in comments next to the tests that print the figures, and in DESIGN.md §3 `berttext`.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402
import sentence_families_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16 = 1, 0
HEADS, RADIUS = 2, 128
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    for key in [k for k in _cache if k[0] == "model"]:
        _cache.pop(key).close()
    c.close()


@pytest.fixture(scope="module")
def emb_mod():
    from marie_icr_amd import embeddings

    return embeddings


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


def _qkv(npad, hd, B=6, heads=HEADS):
    """the input recipe of tests/test_berttext_gpu.py: three different draws, a ramp over the position on k and over the head dim
    on v"""
    rng = np.random.default_rng(1000 * hd + npad)
    D = heads * hd
    q = rng.standard_normal((B, npad, D)) * (R.LOG2E / np.sqrt(hd))
    k = rng.standard_normal((B, npad, D)) + 0.3 * np.linspace(-1, 1, npad)[None, :, None]
    v = rng.standard_normal((B, npad, D)) + np.linspace(-1, 1, D)[None, None, :]
    return [np.ascontiguousarray(a, np.float32) for a in (q, k, v)]


def _table():
    """random, asymmetric in the distance and different per head, within +-4 (log2 units): a sign or off-by-one error in i - j
    moves the scores by units"""
    t = np.random.default_rng(77).uniform(-4.0, 4.0, (HEADS, 2 * RADIUS + 1)).astype(np.float32)
    assert np.abs(t[:, :RADIUS] - t[:, :RADIUS:-1]).mean() > 1.0
    return t


TABLE = _table()


def _attention_case(npad, lens, hd, f16):
    """float64 reference or its f16 emulation, computed once and left unchanged"""
    key = ("attn", npad, tuple(lens), hd, f16)
    if key not in _cache:
        q, k, v = _qkv(npad, hd, B=len(lens))
        if f16:
            out = R.r16(S.attention(R.r16(q), R.r16(k), R.r16(v), lens, HEADS, TABLE, f16=True))
        else:
            out = S.attention(*(a.astype(np.float64) for a in (q, k, v)), lens, HEADS, TABLE)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- 1. the attention alone
# lengths: below a 16-key tile, the tile's edge, the edge + 1, a tile and a half, 113 = 7 tiles + 1 and full; npad 8 and 24 hold what fits
# first MI355X run: f32 5.9e-7 .. 1.5e-6; f16 max |kernel - fp64| 1.50e-3 .. 2.02e-3 over the six cases, equal to E_ref of its case
# to the four digits printed
@pytest.mark.parametrize("npad", [8, 24, 128])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_short_with_a_table(ctx, emb_mod, precision, hd, npad):
    lens = np.array([min(n, npad) for n in (3, 16, 17, 24, 113, 128)], np.int32)
    q, k, v = _qkv(npad, hd)
    want = _attention_case(npad, lens, hd, False)
    got = emb_mod.short_attention_rel_host(ctx, precision, q, k, v, lens, HEADS, TABLE)
    err = np.abs(got - want).max()
    assert 0.5 <= np.abs(want).max() <= 8 and np.isfinite(got).all()
    plain = R.attention(*(a.astype(np.float64) for a in (q, k, v)), lens, HEADS)
    assert np.abs(plain - want).max() > 0.1                              # the table is no small term
    if precision == F32:
        print(f"attn_short rel f32 hd {hd} npad {npad}: max |d| {err:.3e}")
        assert err <= 1e-3
    else:
        e_ref = np.abs(_attention_case(npad, lens, hd, True) - want).max()
        print(f"attn_short rel f16 hd {hd} npad {npad}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        assert err <= 2 * e_ref


# first MI355X run: f32 8.5e-7 .. 1.5e-6; f16 6.5e-4 .. 1.15e-3 over the eight cases, equal to E_ref to the four digits printed
# a single block through the streamed code; the block edge, edge + 1 and + 3; a third block of one key; 5 key blocks and 9 query blocks
LONG_SHAPES = [(128, (128,)), (136, (128, 129, 131)), (264, (128, 129, 131, 257)), (520, (513,))]


def _computed(lens, npad):
    """bool (B, npad): the rows attn_long computes — those of the 64-query blocks that start below the length"""
    return np.arange(npad)[None, :] < (np.asarray(lens)[:, None] + 63) // 64 * 64


@pytest.mark.parametrize("npad,lens", LONG_SHAPES, ids=[f"npad{n}" for n, _ in LONG_SHAPES])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_long_with_a_table(ctx, emb_mod, precision, hd, npad, lens):
    lens = np.array(lens, np.int32)
    q, k, v = _qkv(npad, hd, B=len(lens))
    want = _attention_case(npad, lens, hd, False)
    got = emb_mod.long_attention_rel_host(ctx, precision, q, k, v, lens, HEADS, TABLE)
    rows = _computed(lens, npad)
    err = np.abs(got - want)[rows].max()
    if precision == F32:
        print(f"attn_long rel f32 hd {hd} npad {npad}: max |d| {err:.3e} (outputs up to {np.abs(want[rows]).max():.2f})")
    else:
        e_ref = np.abs(_attention_case(npad, lens, hd, True) - want)[rows].max()
        print(f"attn_long rel f16 hd {hd} npad {npad}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    assert 0.5 <= np.abs(want[rows]).max() <= 8 and np.isfinite(got).all()
    assert err <= (1e-3 if precision == F32 else 2 * e_ref)
    assert (got[~rows] == 0).all()


def test_the_table_is_read_at_query_minus_key(ctx, emb_mod):
    """exact data: q = 0, so the scores are the table alone, and one-hot values read the probabilities back.  Distances up to 199
    on both sides: the clamp at +-128, in the whole-row kernel (24 rows) and across two key blocks of the streamed one"""
    hd = 64
    for npad, n, entry in ((24, 20, emb_mod.short_attention_rel_host), (200, 200, emb_mod.long_attention_rel_host)):
        for first in range(0, n, hd):
            q = np.zeros((1, npad, HEADS * hd), np.float32)
            k = np.ones_like(q)
            v = np.zeros_like(q)
            width = min(hd, n - first)
            for h in range(HEADS):
                v[0, first + np.arange(width), h * hd + np.arange(width)] = 1.0      # value d of key first + d is 1
            got = entry(ctx, F32, q, k, v, [n], HEADS, TABLE)
            i, j = np.meshgrid(np.arange(npad), np.arange(n), indexing="ij")
            for h in range(HEADS):
                full = np.exp2(TABLE[h].astype(np.float64)[np.clip(i - j, -RADIUS, RADIUS) + RADIUS])
                want = full[:, first:first + width] / full.sum(-1, keepdims=True)
                err = np.abs(got[0, :, h * hd:h * hd + width] - want).max()
                print(f"table probabilities npad {npad} keys {first} .. {first + width - 1} head {h}: max |d| {err:.3e}")
                assert err <= 1e-6


# ---------------------------------------------------------------------------------------------------- 2. bit invariance
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("streamed", [False, True], ids=["short", "long"])
def test_rows_with_a_table_depend_on_the_sequence_alone_bitwise(ctx, emb_mod, precision, streamed):
    hd = 32
    entry = emb_mod.long_attention_rel_host if streamed else emb_mod.short_attention_rel_host
    small, wide = (136, 264) if streamed else (24, 128)
    lens = np.array([3, 129, 131, 136, 64, 17] if streamed else [3, 16, 17, 24, 1, 9], np.int32)
    q, k, v = _qkv(small, hd)
    got = entry(ctx, precision, q, k, v, lens, HEADS, TABLE)
    # what lies past a sequence's length does not reach it
    k2, v2 = k.copy(), v.copy()
    for b, n in enumerate(lens):
        k2[b, n:] = k2[b, n:] * -1.5 + 2.0
        v2[b, n:] += 3.0
    assert np.array_equal(entry(ctx, precision, q, k2, v2, lens, HEADS, TABLE), got)
    # the same sequences in wider rows: rows < len are the same bits
    more = _qkv(wide - small, hd)
    wq, wk, wv = (np.ascontiguousarray(np.concatenate([a, m], 1)) for a, m in zip((q, k, v), more))
    far = entry(ctx, precision, wq, wk, wv, lens, HEADS, TABLE)
    for b, n in enumerate(lens):
        assert np.array_equal(far[b, :n], got[b, :n]), f"sequence {b} of {n} keys depends on npad"
    # and alone in its own batch
    b, n = 2, int(lens[2])
    own = (n + 7) // 8 * 8
    alone = entry(ctx, precision, q[b:b + 1, :own], k[b:b + 1, :own], v[b:b + 1, :own], lens[b:b + 1], HEADS, TABLE)
    assert np.array_equal(alone[0, :n], got[b, :n])


@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_a_null_table_is_the_plain_entry_bitwise(ctx, emb_mod, precision):
    for hd in (32, 64):
        lens = np.array([3, 16, 17, 24, 113, 128], np.int32)
        q, k, v = _qkv(128, hd)
        assert np.array_equal(emb_mod.short_attention_rel_host(ctx, precision, q, k, v, lens, HEADS, None),
                              emb_mod.short_attention_host(ctx, precision, q, k, v, lens, HEADS))
        lens = np.array([128, 129, 131, 257, 3, 264], np.int32)
        q, k, v = _qkv(264, hd)
        assert np.array_equal(emb_mod.long_attention_rel_host(ctx, precision, q, k, v, lens, HEADS, None),
                              emb_mod.long_attention_host(ctx, precision, q, k, v, lens, HEADS))
    # a table of zeros adds 0.0 to every score: the same bits through the other instances
    zeros = np.zeros_like(TABLE)
    assert np.array_equal(emb_mod.long_attention_rel_host(ctx, precision, q, k, v, lens, HEADS, zeros),
                          emb_mod.long_attention_host(ctx, precision, q, k, v, lens, HEADS))


# ---------------------------------------------------------------------------------------------------- 3. the embedding kernel
@pytest.mark.parametrize("B,npad,D,vocab", [(3, 8, 64, 50), (5, 40, 384, 300), (2, 24, 1024, 7)])
def test_embed_kernel_with_offset_and_without_types(ctx, emb_mod, B, npad, D, vocab):
    rng = np.random.default_rng(B * D)
    word, pos = rng.standard_normal((vocab, D)).astype(np.float32), rng.standard_normal((npad + 2, D)).astype(np.float32)
    type0 = (0.5 * rng.standard_normal(D)).astype(np.float32)
    g, b = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32), (0.2 * rng.standard_normal(D)).astype(np.float32)
    ids = rng.integers(0, vocab, (B, npad)).astype(np.int32)
    ids[0, 0], ids[0, 1], ids[-1, -1], ids[-1, 0] = 0, vocab - 1, vocab - 1, 0
    got = emb_mod.bert_embed_rows_ex_host(ctx, word, None, pos, g, b, ids, eps=1e-5, pos_offset=2)
    want = R.layer_norm(word.astype(np.float64)[ids] + pos.astype(np.float64)[2:], g.astype(np.float64), b.astype(np.float64), 1e-5)
    err = np.abs(got - want).max()
    print(f"berttext_embed B {B} npad {npad} D {D} offset 2, no types: max |d| {err:.3e} (entries up to {np.abs(want).max():.2f})")
    assert err <= 1e-3
    assert np.abs(want - R.layer_norm(word.astype(np.float64)[ids] + pos.astype(np.float64)[:npad], g.astype(np.float64),
                                      b.astype(np.float64), 1e-5)).max() > 0.5      # the offset is no small matter
    # offset 0 with a type row: the entry that was there, bit for bit
    assert np.array_equal(emb_mod.bert_embed_rows_ex_host(ctx, word, type0, pos[:npad], g, b, ids, eps=1e-12, pos_offset=0),
                          emb_mod.bert_embed_rows_host(ctx, word, type0, pos[:npad], g, b, ids, eps=1e-12))


# ---------------------------------------------------------------------------------------------------- 4. the encoders
NAMES = list(S.MODELS) + ["mpnet_b_long"]


def _cfg(name):
    return S.MODELS["mpnet_b" if name == "mpnet_b_long" else name]


def _reference(golden, name, mode="mean", normalize=False, f16=False):
    key = ("ref", name, mode, normalize, f16)
    if key not in _cache:
        g = golden[0][name]
        taps, emb = S.forward(g["state"], _cfg(name), g["ids"], g["lens"], golden[1], mode, normalize, f16)
        taps.setflags(write=False)
        emb.setflags(write=False)
        _cache[key] = (taps, emb)
    return _cache[key]


def _model(ctx, emb_mod, golden, name, precision, mode="mean", normalize=False):
    base = "mpnet_b" if name == "mpnet_b_long" else name
    key = ("model", base, precision, mode, normalize)
    if key not in _cache:
        tensors, cfg, _ = emb_mod.load_sentence_encoder_state(golden[0][base]["state"], S.config_json(S.MODELS[base]))
        cfg.pool, cfg.normalize = (emb_mod.POOL_CLS if mode == "cls" else emb_mod.POOL_MEAN), int(normalize)
        _cache[key] = emb_mod.BertTextModel(ctx, tensors, cfg, precision)
    return _cache[key]


def _all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


@pytest.mark.parametrize("name", NAMES)
def test_fp32_taps_embeddings_and_cosines(ctx, emb_mod, golden, name):
    g = golden[0][name]
    ids, lens = g["ids"], g["lens"]
    valid = R.valid_rows(lens, ids.shape[1])
    ref_taps, _ = _reference(golden, name)
    assert 0.5 <= np.abs(ref_taps[:, valid]).max() <= 10
    m = _model(ctx, emb_mod, golden, name, F32)
    taps, emb = m.debug_taps_host(ids, lens)
    assert np.isfinite(taps).all()                                   # the rows nobody reads too
    tap_err = [float(np.abs(taps[i] - ref_taps[i])[valid].max()) for i in range(len(taps))]
    rows_err = np.abs(S.take_rows(taps, g["rows"]) - g["hidden_rows"]).max()
    print(f"{name} fp32 npad {ids.shape[1]}: taps {' '.join(f'{e:.2e}' for e in tap_err)}; the golden's hidden rows {rows_err:.3e}")
    for i, e in enumerate(tap_err):
        assert e <= 1e-3, f"tap {i} (0: the embedding kernel, k: layer k)"
    assert rows_err <= 1e-3
    for mode, norm, stored in (("mean", False, "mean"), ("mean", True, "mean_norm"), ("cls", False, "cls")):      # what transformers computed
        mm = _model(ctx, emb_mod, golden, name, F32, mode, norm)
        cos, got = mm.embed_pairs_host(ids, lens, _all_pairs(len(ids)), want_embeddings=True)
        ref_cos = R.cosine_matrix(g[stored])
        emb_err, cos_err = np.abs(got - g[stored]).max(), np.abs(cos.reshape(ref_cos.shape) - ref_cos).max()
        print(f"{name} fp32 {mode}{' normalized' if norm else ''}: embeddings {emb_err:.3e} (entries up to {np.abs(g[stored]).max():.2f}); "
              f"cosines {cos_err:.3e} ({ref_cos.min():.3f} .. 1)")
        assert emb_err <= 1e-3 and cos_err <= 1e-5
        assert np.array_equal(got, mm.embed_ids_host(ids, lens))
        if (mode, norm) == ("mean", False):
            assert np.array_equal(got, emb)


# first MI355X run, max |kernel - fp64| (E_ref) for the taps after layer 1 and 2, the embeddings, the cosines:
#   mpnet_a       3.24e-3 (3.24e-3)   7.53e-3 (7.53e-3)    1.28e-3 (1.39e-3)   8.6e-5 (8.9e-5)
#   mpnet_b       4.82e-3 (4.82e-3)   6.69e-3 (6.85e-3)    1.94e-3 (1.94e-3)   3.7e-5 (3.6e-5)
#   roberta       3.72e-3 (3.33e-3)   1.117e-2 (1.032e-2)  1.69e-3 (1.69e-3)   1.30e-4 (1.39e-4)
#   distilbert    4.69e-3 (4.69e-3)   1.000e-2 (1.000e-2)  1.19e-3 (1.19e-3)   1.35e-4 (1.15e-4)
#   mpnet_b_long  6.64e-3 (6.64e-3)   8.41e-3 (9.48e-3)    6.8e-4 (8.2e-4)     4.1e-5 (4.2e-5)
# (fp32 mode on the same cases: taps <= 8.0e-6, embeddings <= 3.9e-6, cosines <= 7.7e-7)
@pytest.mark.parametrize("name", NAMES)
def test_f16_within_twice_the_emulated_rounding_error(ctx, emb_mod, golden, name):
    g = golden[0][name]
    ids, lens = g["ids"], g["lens"]
    valid = R.valid_rows(lens, ids.shape[1])
    ref_taps, ref_emb = _reference(golden, name)
    emu_taps, emu_emb = _reference(golden, name, f16=True)
    m = _model(ctx, emb_mod, golden, name, F16)
    taps, emb = m.debug_taps_host(ids, lens)
    assert np.isfinite(taps).all()
    checks = []
    for i in range(len(taps)):
        err, e_ref = np.abs(taps[i] - ref_taps[i])[valid].max(), np.abs(emu_taps[i] - ref_taps[i])[valid].max()
        print(f"{name} f16 tap {i}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        checks.append((f"tap {i}", err, 1e-3 if i == 0 else 2 * e_ref))      # nothing is rounded to f16 before the first GEMM
    err, e_ref = np.abs(emb - ref_emb).max(), np.abs(emu_emb - ref_emb).max()
    print(f"{name} f16 embeddings: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    checks.append(("embeddings", err, 2 * e_ref))
    cos = m.embed_pairs_host(ids, lens, _all_pairs(len(ids))).reshape(len(ids), len(ids))
    ref_cos, emu_cos = R.cosine_matrix(ref_emb), R.cosine_matrix(emu_emb)
    err, e_ref = np.abs(cos - ref_cos).max(), np.abs(emu_cos - ref_cos).max()
    print(f"{name} f16 cosines: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    checks.append(("cosines", err, 2 * e_ref))
    for what, err, bar in checks:
        assert err <= bar, what


# ---------------------------------------------------------------------------------------------------- 5. the public classes
WORDS = ["the", "invoice", "amount", "due", "pay", "no", "12", "resume"]      # one WordPiece piece each, and one BPE token after a blank


def _texts(counts, seed):
    """texts of `counts` words, "the" first (one BPE token without a blank before it too): counts + 2 tokens in both tokenizers"""
    rng = np.random.default_rng(seed)
    return [" ".join(["the"] + [WORDS[j] for j in rng.integers(0, len(WORDS), c - 1)]) for c in counts]


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("family", ["mpnet", "roberta"])
def test_embed_texts_equals_the_single_texts(ctx, emb_mod, golden, tmp_path, family, precision):
    from marie_icr_amd.document_classifier import ByteLevelBPE
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    if family == "mpnet":      # the golden's weights: 520 position rows
        cfg, state = S.MODELS["mpnet_b"], golden[0]["mpnet_b"]["state"]
        tok = WordPieceTokenizer(S.MPNET_VOCAB, cls_token="<s>", sep_token="</s>", pad_token="<pad>", mask_token="<mask>")
    else:                      # the golden's RoBERTa has 136 position rows: seeded weights with 264
        cfg = dict(S.MODELS["roberta"], max_position=264)
        state = R.quantize_state(S.make_state(cfg, 31))[0]
        tok = ByteLevelBPE(*S.write_bpe_files(str(tmp_path)))
    e = emb_mod.SentenceTransformerEmbeddings(state=state, config=S.config_json(cfg), tokenizer=tok, precision=precision, ctx=ctx,
                                              max_seq_length=cfg["max_position"])
    try:
        assert e.family == family and e.max_tokens == cfg["max_position"] - 2 and (e.pooling, e.normalize) == ("mean", True)
        rng = np.random.default_rng(5)
        counts = [1, 2, 14, 15, 126, 127, 128, 129, 134, 198] + [int(c) for c in rng.integers(1, 199, 20)]
        texts = _texts(counts, 9)
        lengths = [len(ids) for ids in e.encode_texts(texts)]
        assert lengths == [c + 2 for c in counts] and min(lengths) == 3 and max(lengths) == 200
        whole = e.embed_texts(texts, chunk=8)
        assert whole.shape == (30, 128) and np.isfinite(whole).all()
        for i, text in enumerate(texts):
            assert np.array_equal(e.embed_texts([text])[0], whole[i]), f"text {i} of {lengths[i]} tokens depends on its batch"
        print(f"embed_texts {family} {precision}: 30 texts of {min(lengths)} .. {max(lengths)} tokens: equal bits alone")
        if precision == "f32":
            ids, lens = tok.pad(e.encode_texts(texts), 200)
            err = np.abs(whole - S.forward(state, cfg, ids, lens, golden[1], "mean", True)[1]).max()
            print(f"embed_texts {family} f32: max |d| {err:.3e}")
            assert err <= 1e-3
        with pytest.raises(ValueError, match="too long"):
            e.embed_texts([" ".join(["invoice"] * (cfg["max_position"] - 3))])
    finally:
        e.close()


def test_meta_template_matcher_takes_an_mpnet_directory(ctx, emb_mod, golden, tmp_path):
    import json

    from safetensors.numpy import save_file

    from marie_icr_amd.template_matching import MetaTemplateMatcher

    cfg, state = S.MODELS["mpnet_b"], golden[0]["mpnet_b"]["state"]
    d = str(tmp_path)
    save_file({"mpnet." + k: v for k, v in state.items()}, os.path.join(d, "model.safetensors"))
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(S.config_json(cfg), f)
    with open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(S.MPNET_VOCAB) + "\n")
    e = emb_mod.SentenceTransformerEmbeddings(d, precision="f32", ctx=ctx)
    try:
        assert (e.family, e.pooling, e.normalize, e.max_seq_length, e.max_tokens) == ("mpnet", "mean", True, 256, 256)
        matcher = MetaTemplateMatcher(embeddings_processor=lambda clip: np.ones(4), text_embeddings_processor=e, ctx=ctx)
        pairs = [("INVOICE TOTAL", "INVOICE TOTAL"), ("TOTAL DUE", "INVOICE TOTAL"), ("PAYMENT DATE", "INVOICE TOTAL")]
        sims = matcher.text_sims(pairs)
        texts = list(dict.fromkeys(t for p in pairs for t in p))
        ids, lens = e.tokenizer.pad([e.tokenizer.encode(t) for t in texts], 8)
        cos = R.cosine_matrix(S.forward(state, cfg, ids, lens, golden[1], "mean", True)[1])
        want = [cos[texts.index(a), texts.index(b)] for a, b in pairs]
        err = np.abs(np.array(sims) - np.array(want)).max()
        print(f"MetaTemplateMatcher.text_sims over MPNet: {np.round(sims, 4)}, max |d cosine| {err:.3e}")
        assert sims[0] == 1.0 and err <= 1e-5
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(ctx, emb_mod, golden):
    from marie_icr_amd._lib import MarieHipError, SentenceEncoderConfig

    good = dict(vocab=80, max_position=136, type_vocab=0, dim=128, heads=2, depth=2, ffn=128, ln_eps=1e-5, position=0, mlp=0, pool=0,
                normalize=0, pos_offset=2, rel_buckets=32, rel_max_distance=128)
    m = _model(ctx, emb_mod, golden, "mpnet_a", F32)                   # 136 position rows, offset 2: 134 tokens
    ctx.profile_enable(True)
    ctx.profile_reset()
    # slopes and a table together; fields out of range
    for change, field in ((dict(position=1, pos_offset=0), "rel_buckets"), (dict(rel_buckets=31), "rel_buckets"), (dict(rel_buckets=2), "rel_buckets"),
                          (dict(rel_max_distance=0), "rel_max_distance"), (dict(rel_buckets=0), "rel_max_distance"), (dict(pos_offset=-1), "pos_offset"),
                          (dict(pos_offset=135), "pos_offset"), (dict(position=1, rel_buckets=0, rel_max_distance=0), "pos_offset"),
                          (dict(type_vocab=-1), "type_vocab")):
        with pytest.raises(MarieHipError, match=field):
            emb_mod.BertTextModel(ctx, None, SentenceEncoderConfig(**dict(good, **change)), F32)
    # the twelve-field entry keeps requiring a token type table
    from marie_icr_amd._lib import BertTextConfig

    with pytest.raises(MarieHipError, match="type_vocab"):
        emb_mod.BertTextModel(ctx, None, BertTextConfig(**{k: v for k, v in good.items() if k not in ("pos_offset", "rel_buckets", "rel_max_distance")}), F32)
    # pos_offset + npad past the table (134 tokens round up to 136 rows), and a text that fills the rows past it
    with pytest.raises(MarieHipError, match="rows a text"):
        m.embed_ids_host(np.full((1, 144), 5, np.int32), [100])
    assert m.workspace_bytes(1, 144) == 0 and m.workspace_bytes(1, 136) > 0
    with pytest.raises(MarieHipError, match="tokens"):
        m.embed_ids_host(np.full((1, 136), 5, np.int32), [135])
    # a table whose buckets do not saturate, a non-finite weight: finalize names them
    tensors, cfg, _ = emb_mod.load_sentence_encoder_state(golden[0]["mpnet_a"]["state"], S.config_json(S.MODELS["mpnet_a"]))
    cfg.rel_max_distance = 8
    with pytest.raises(MarieHipError, match="rel_max_distance"):
        emb_mod.BertTextModel(ctx, tensors, cfg, F32)
    cfg.rel_max_distance = 128
    bad = dict(tensors)
    bad["encoder.relative_attention_bias.weight"] = tensors["encoder.relative_attention_bias.weight"].copy()
    bad["encoder.relative_attention_bias.weight"][3, 1] = np.inf
    with pytest.raises(MarieHipError, match="non-finite"):
        emb_mod.BertTextModel(ctx, bad, cfg, F32)
    del bad["encoder.relative_attention_bias.weight"]
    with pytest.raises(MarieHipError, match=r"encoder\.relative_attention_bias\.weight"):
        emb_mod.BertTextModel(ctx, bad, cfg, F32)
    # the kernel entries: a non-finite table, more rows than the whole-row kernel holds
    q = np.zeros((1, 8, 64), np.float32)
    table = TABLE.copy()
    table[1, 7] = -np.inf
    with pytest.raises(MarieHipError, match="non-finite"):
        emb_mod.short_attention_rel_host(ctx, F32, q, q, q, [8], HEADS, table)
    x = np.zeros((1, 136, 64), np.float32)
    with pytest.raises(MarieHipError):
        emb_mod.short_attention_rel_host(ctx, F32, x, x, x, [136], HEADS, TABLE)
    after = ctx.profile_read()
    ctx.profile_enable(False)
    assert all(after[k]["launches"] == 0 for k in after), {k: v["launches"] for k, v in after.items() if v["launches"]}
    ids, lens = golden[0]["mpnet_a"]["ids"], golden[0]["mpnet_a"]["lens"]
    assert m.embed_ids_host(ids, lens).shape == (4, 64)
