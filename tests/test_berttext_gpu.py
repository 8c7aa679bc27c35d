"""BERT sentence encoders on the MI355X (marie_icr_amd/csrc/berttext_api.hip, berttext_ops.hip, attn_seq.hip) against tests/bert_text_ref.py,
the float64 restatement that tests/test_berttext_cpu.py pins to transformers.BertModel through tests/golden/bert_text.npz.

Bars:
  * the kernels alone against float64, and fp32 mode against the goldens (plain BERT) or the restatement (ALiBi + GEGLU): 1e-3
    absolute on O(1) quantities for stream taps and embeddings, 1e-5 for cosines — the project's bars for the CLIP text tower
    (tests/test_cliptext_gpu.py);
  * f16 mode: for each case E_ref = max |f16-rounded restatement - float64 restatement| is computed here on the CPU, and
    max |kernel - float64 restatement| <= 2 E_ref: the factor allows about one more rounding per stage where the kernel's rounding
    points and accumulation order differ from the emulation;
  * a text's embedding does not depend on npad or on the call it is part of: bitwise, in both precisions.
Every test prints its figures before it asserts.

First MI355X run: recorded in comments next to the tests that print the figures, and in DESIGN.md §3 `berttext`.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_text.npz")
F32, F16 = 1, 0
CONFIGS = {"A": R.CONFIG_A, "B": R.CONFIG_B, "B_jina": R.CONFIG_B_JINA}
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
    return R.load_golden(GOLDEN)


def _case(golden, name):
    """(state, ids, lens) of a case: the goldens' for A and B, seeded JinaBERT weights on B's ids for B_jina"""
    if name == "B_jina":
        if ("state", name) not in _cache:
            _cache[("state", name)] = R.quantize_state(R.make_state(R.CONFIG_B_JINA, 13))[0]
        return _cache[("state", name)], golden[0]["B"]["ids"], golden[0]["B"]["lens"]
    g = golden[0][name]
    return g["state"], g["ids"], g["lens"]


def _reference(golden, name, mode="mean", normalize=False, f16=False):
    """(taps, embeddings) of the restatement, computed once and left unchanged"""
    key = ("ref", name, mode, normalize, f16)
    if key not in _cache:
        state, ids, lens = _case(golden, name)
        taps, emb = R.forward(state, CONFIGS[name], ids, lens, mode, normalize, f16)
        taps.setflags(write=False)
        emb.setflags(write=False)
        _cache[key] = (taps, emb)
    return _cache[key]


def _model(ctx, emb_mod, golden, name, precision, mode="mean", normalize=False):
    key = ("model", name, precision, mode, normalize)
    if key not in _cache:
        state, _, _ = _case(golden, name)
        tensors, cfg = emb_mod.load_bert_text_state(state, R.config_json(CONFIGS[name]))
        cfg.pool, cfg.normalize = (emb_mod.POOL_CLS if mode == "cls" else emb_mod.POOL_MEAN), int(normalize)
        _cache[key] = emb_mod.BertTextModel(ctx, tensors, cfg, precision)
    return _cache[key]


def _all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


# ---------------------------------------------------------------------------------------------------- 1. attn_short alone
def _qkv(npad, hd, B=6, heads=2):
    """asymmetric O(1) inputs: three different draws, a ramp over the position on k and over the head dim on v"""
    rng = np.random.default_rng(1000 * hd + npad)
    D = heads * hd
    q = rng.standard_normal((B, npad, D)) * (R.LOG2E / np.sqrt(hd))
    k = rng.standard_normal((B, npad, D)) + 0.3 * np.linspace(-1, 1, npad)[None, :, None]
    v = rng.standard_normal((B, npad, D)) + np.linspace(-1, 1, D)[None, None, :]
    return [np.ascontiguousarray(a, np.float32) for a in (q, k, v)]


SLOPES = np.array([0.5, 0.0625]) * R.LOG2E      # log2 units, as the encoder passes them


# lengths: a single key, two, below a 16-key tile, the tile's edge, the edge + 1 (the 32-key step of the f16 second product takes a
# zero tile), and full; npad 8 holds what fits
# first MI355X run: f32 4.8e-7 .. 4.0e-6 (largest: npad 128 with ALiBi); f16 max |kernel - fp64| 1.33e-3 .. 2.23e-3 over the twelve
# cases, equal to E_ref of its case to the four digits printed (outputs up to 3.5, whose own f16 rounding is up to 9.8e-4)
@pytest.mark.parametrize("slopes", [None, SLOPES], ids=["plain", "alibi"])
@pytest.mark.parametrize("npad", [8, 24, 128])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_short_kernel(ctx, emb_mod, precision, hd, npad, slopes):
    heads = 2
    lens = np.array([min(n, npad) for n in (1, 2, 7, 16, 17, npad)], np.int32)
    q, k, v = _qkv(npad, hd)
    want = R.attention(*(a.astype(np.float64) for a in (q, k, v)), lens, heads, slopes)
    got = emb_mod.short_attention_host(ctx, precision, q, k, v, lens, heads, slopes)
    err = np.abs(got - want).max()
    assert 0.5 <= np.abs(want).max() <= 8 and np.isfinite(got).all()
    if precision == F32:
        print(f"attn_short f32 hd {hd} npad {npad} {'alibi' if slopes is not None else 'plain'}: max |d| {err:.3e}")
        assert err <= 1e-3
    else:
        emu = R.r16(R.attention(R.r16(q), R.r16(k), R.r16(v), lens, heads, slopes, f16=True))
        e_ref = np.abs(emu - want).max()
        print(f"attn_short f16 hd {hd} npad {npad} {'alibi' if slopes is not None else 'plain'}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        assert err <= 2 * e_ref
    # a sequence of one key returns that key's values, whatever the bias
    want0 = v[0, 0] if precision == F32 else v[0, 0].astype(np.float16).astype(np.float32)
    assert np.array_equal(got[0], np.broadcast_to(want0, got[0].shape))
    # what lies past a sequence's length does not reach it: bitwise, queries past the length included
    k2, v2 = k.copy(), v.copy()
    for b, n in enumerate(lens):
        k2[b, n:] = k2[b, n:] * -1.5 + 2.0
        v2[b, n:] += 3.0
    assert np.array_equal(emb_mod.short_attention_host(ctx, precision, q, k2, v2, lens, heads, slopes), got)
    # and a sequence does not depend on its batch or on npad
    if npad > 8:
        b, n = 2, 8
        alone = emb_mod.short_attention_host(ctx, precision, q[b:b + 1, :n], k[b:b + 1, :n], v[b:b + 1, :n], lens[b:b + 1], heads, slopes)
        assert np.array_equal(alone[0, :lens[b]], got[b, :lens[b]])


def test_attn_short_bias_is_the_symmetric_distance(ctx, emb_mod):
    """exact data: q = 0, so the scores are the bias alone, and one-hot values read the probabilities back"""
    npad, hd, heads = 24, 32, 2
    q = np.zeros((1, npad, heads * hd), np.float32)
    k = np.ones_like(q)
    v = np.zeros_like(q)
    v[0, np.arange(npad), np.arange(npad)] = 1.0                    # head 0: value d of key j is [d == j], keys 0 .. 23 < 32
    v[0, np.arange(npad), hd + np.arange(npad)] = 1.0               # head 1
    lens = np.array([20], np.int32)
    got = emb_mod.short_attention_host(ctx, F32, q, k, v, lens, heads, SLOPES)
    for h in range(heads):
        p = got[0, :, h * hd:h * hd + npad].astype(np.float64)      # p[i, j]
        i, j = np.meshgrid(np.arange(npad), np.arange(npad), indexing="ij")
        want = np.where(j < 20, np.exp2(-SLOPES[h] * np.abs(i - j)), 0.0)
        want /= want.sum(-1, keepdims=True)
        assert np.abs(p - want).max() <= 1e-6, f"head {h}"
        assert (p[:, 20:] == 0).all()


# ---------------------------------------------------------------------------------------------------- 2. the other kernels
@pytest.mark.parametrize("with_pos", [True, False], ids=["positions", "no-positions"])
@pytest.mark.parametrize("B,npad,D,vocab", [(3, 8, 64, 50), (5, 40, 384, 300), (2, 24, 1024, 7)])
def test_embed_kernel(ctx, emb_mod, B, npad, D, vocab, with_pos):
    rng = np.random.default_rng(B * D + with_pos)
    word, pos = rng.standard_normal((vocab, D)).astype(np.float32), rng.standard_normal((npad, D)).astype(np.float32)
    type0 = (0.5 * rng.standard_normal(D)).astype(np.float32)
    g, b = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32), (0.2 * rng.standard_normal(D)).astype(np.float32)
    ids = rng.integers(0, vocab, (B, npad)).astype(np.int32)
    ids[0, 0], ids[0, 1], ids[-1, -1], ids[-1, 0] = 0, vocab - 1, vocab - 1, 0
    got = emb_mod.bert_embed_rows_host(ctx, word, type0, pos if with_pos else None, g, b, ids, eps=1e-12)
    x = word.astype(np.float64)[ids] + type0.astype(np.float64) + (pos.astype(np.float64) if with_pos else 0.0)
    want = R.layer_norm(x, g.astype(np.float64), b.astype(np.float64), 1e-12)
    err = np.abs(got - want).max()
    print(f"berttext_embed B {B} npad {npad} D {D} {'with' if with_pos else 'without'} positions: max |d| {err:.3e} "
          f"(entries up to {np.abs(want).max():.2f})")
    assert err <= 1e-3


@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("R_,F", [(3, 64), (17, 1536), (130, 256)])
def test_geglu_kernel(ctx, emb_mod, precision, R_, F):
    rng = np.random.default_rng(R_ * F)
    x = (2.0 * rng.standard_normal((R_, 2 * F))).astype(np.float32)
    x[0, :4], x[0, F:F + 4] = [0.0, -6.0, 6.0, 1e-3], [1.0, 1.0, -1.0, 2.0]
    got = emb_mod.geglu_host(ctx, precision, x)
    xs = x.astype(np.float64)
    want = R.gelu(xs[:, :F]) * xs[:, F:]
    err = np.abs(got - want).max()
    if precision == F32:
        print(f"geglu f32 R {R_} F {F}: max |d| {err:.3e} (entries up to {np.abs(want).max():.1f})")
        assert err <= 1e-3
    else:
        x16 = R.r16(x)
        e_ref = np.abs(R.r16(R.gelu(x16[:, :F]) * x16[:, F:]) - want).max()
        print(f"geglu f16 R {R_} F {F}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        assert err <= 2 * e_ref


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("mode", ["mean", "cls"])
@pytest.mark.parametrize("npad,D", [(8, 64), (24, 384), (128, 1024)])
def test_pool_kernel(ctx, emb_mod, npad, D, mode, normalize):
    rng = np.random.default_rng(npad + D)
    lens = np.array([1, npad, min(7, npad), npad - 1, 1], np.int32)
    h = (rng.standard_normal((len(lens), npad, D)) + 0.5).astype(np.float32)
    h[-1, 0] = 0.0                                                   # a zero row: the normalisation's floor, not a division by zero
    code = emb_mod.POOL_CLS if mode == "cls" else emb_mod.POOL_MEAN
    got = emb_mod.bert_pool_host(ctx, h, lens, code, normalize)
    want = R.pool(h.astype(np.float64), lens, mode, normalize)
    err = np.abs(got - want).max()
    print(f"berttext_pool {mode} normalize {normalize} npad {npad} D {D}: max |d| {err:.3e}")
    assert err <= 1e-3      # a length off by one moves a mean by 0.5 / 128 = 4e-3
    assert np.isfinite(got).all() and (got[-1] == 0).all()
    # rows past the length are not read: bitwise
    h2 = h.copy()
    for b, n in enumerate(lens):
        h2[b, n:] = np.nan
    assert np.array_equal(emb_mod.bert_pool_host(ctx, h2, lens, code, normalize), got)


# ---------------------------------------------------------------------------------------------------- 3. fp32 encoders
@pytest.mark.parametrize("name", ["A", "B", "B_jina"])
def test_fp32_taps_embeddings_and_cosines(ctx, emb_mod, golden, name):
    state, ids, lens = _case(golden, name)
    valid = R.valid_rows(lens, ids.shape[1])
    if name == "B_jina":
        ref_taps, _ = _reference(golden, name)
        want = {(m, n): _reference(golden, name, m, n)[1] for m, n in (("mean", False), ("mean", True), ("cls", False))}
    else:      # what transformers computed
        g = golden[0][name]
        ref_taps, want = g["hidden"], {("mean", False): g["mean"], ("mean", True): g["mean_norm"], ("cls", False): g["cls"]}
    assert 0.5 <= np.abs(ref_taps).max() <= 10
    m = _model(ctx, emb_mod, golden, name, F32)
    taps, emb = m.debug_taps_host(ids, lens)
    assert np.isfinite(taps).all()                                   # the rows nobody reads too
    tap_err = [float(np.abs(taps[i] - ref_taps[i])[valid].max()) for i in range(len(taps))]
    print(f"{name} fp32: taps {' '.join(f'{e:.2e}' for e in tap_err)}")
    for i, e in enumerate(tap_err):
        assert e <= 1e-3, f"tap {i} (0: the embedding kernel, k: layer k)"
    for (mode, norm), ref_emb in want.items():
        mm = _model(ctx, emb_mod, golden, name, F32, mode, norm)
        cos, got = mm.embed_pairs_host(ids, lens, _all_pairs(len(ids)), want_embeddings=True)
        ref_cos = R.cosine_matrix(ref_emb)
        emb_err, cos_err = np.abs(got - ref_emb).max(), np.abs(cos.reshape(ref_cos.shape) - ref_cos).max()
        print(f"{name} fp32 {mode}{' normalized' if norm else ''}: embeddings {emb_err:.3e} (entries up to {np.abs(ref_emb).max():.2f}); "
              f"cosines {cos_err:.3e} ({ref_cos.min():.3f} .. 1)")
        assert emb_err <= 1e-3 and cos_err <= 1e-5
        assert np.array_equal(got, mm.embed_ids_host(ids, lens))
        if (mode, norm) == ("mean", False):
            assert np.array_equal(got, emb)
    assert m.workspace_bytes(len(ids), ids.shape[1]) > 0 and m.workspace_bytes(len(ids), ids.shape[1] + 1) == 0


# ---------------------------------------------------------------------------------------------------- 4. f16 encoders
# first MI355X run, max |kernel - fp64| (E_ref) for the taps after layer 1 and 2, the embeddings, the cosines:
#   A       4.58e-3 (4.58e-3)   4.43e-3 (4.57e-3)   8.33e-4 (8.19e-4)   4.7e-5 (4.8e-5)
#   B       4.43e-3 (4.43e-3)   5.79e-3 (6.53e-3)   1.31e-3 (1.31e-3)   9.5e-5 (9.4e-5)
#   B_jina  4.06e-3 (4.06e-3)   7.61e-3 (8.34e-3)   1.50e-3 (1.59e-3)   1.02e-4 (9.0e-5)
# (stream entries up to 6.7; fp32 mode on the same cases: taps <= 7.7e-6, embeddings <= 2.8e-6, cosines <= 2.9e-7)
@pytest.mark.parametrize("name", ["A", "B", "B_jina"])
def test_f16_within_twice_the_emulated_rounding_error(ctx, emb_mod, golden, name):
    _, ids, lens = _case(golden, name)
    valid = R.valid_rows(lens, ids.shape[1])
    ref_taps, ref_emb = _reference(golden, name)
    emu_taps, emu_emb = _reference(golden, name, f16=True)
    m = _model(ctx, emb_mod, golden, name, F16)
    taps, emb = m.debug_taps_host(ids, lens)
    assert np.isfinite(taps).all()
    for i in range(len(taps)):
        err, e_ref = np.abs(taps[i] - ref_taps[i])[valid].max(), np.abs(emu_taps[i] - ref_taps[i])[valid].max()
        print(f"{name} f16 tap {i}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        if i == 0:
            assert err <= 1e-3                                       # nothing is rounded to f16 before the first GEMM
        else:
            assert err <= 2 * e_ref
    err, e_ref = np.abs(emb - ref_emb).max(), np.abs(emu_emb - ref_emb).max()
    print(f"{name} f16 embeddings: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    assert err <= 2 * e_ref
    cos = m.embed_pairs_host(ids, lens, _all_pairs(len(ids))).reshape(len(ids), len(ids))
    ref_cos, emu_cos = R.cosine_matrix(ref_emb), R.cosine_matrix(emu_emb)
    err, e_ref = np.abs(cos - ref_cos).max(), np.abs(emu_cos - ref_cos).max()
    # for comparison only: a cosine moves by at most |dx| / |x| + |dy| / |y|, and an embedding entry by at most 2 E_ref (above)
    loose = 2 * 2 * np.abs(emu_emb - ref_emb).max() * np.sqrt(ref_emb.shape[1]) / np.sqrt((ref_emb ** 2).sum(-1)).min()
    print(f"{name} f16 cosines: max |d| {err:.3e}, E_ref {e_ref:.3e} (what the embedding bound alone would allow: {loose:.3e})")
    assert err <= 2 * e_ref


# ---------------------------------------------------------------------------------------------------- 5. batch independence
@pytest.mark.parametrize("name", ["A", "B_jina"])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_a_text_does_not_depend_on_npad_or_its_batch_bitwise(ctx, emb_mod, golden, precision, name):
    _, ids, lens = _case(golden, name)
    m = _model(ctx, emb_mod, golden, name, precision)
    together = m.embed_ids_host(ids, lens)
    for i, n in enumerate(lens):
        own = (int(n) + 7) // 8 * 8
        alone = m.embed_ids_host(ids[i:i + 1, :own], lens[i:i + 1])
        wide = np.zeros((1, 128), np.int32)
        wide[0, :ids.shape[1]] = ids[i]
        assert np.array_equal(alone[0], together[i]), f"text {i} of {n} tokens depends on its batch"
        assert np.array_equal(m.embed_ids_host(wide, lens[i:i + 1])[0], together[i]), f"text {i} of {n} tokens depends on npad"
    print(f"{name}: texts of {[int(n) for n in lens]} tokens alone at their own npad, together at {ids.shape[1]} and alone at 128 rows: equal bits")
    assert np.abs(together[0] - together[1]).max() > 1e-3


# ---------------------------------------------------------------------------------------------------- 6. the public surface
WORDS = ["the", "invoice", "total", "amount", "due", "date", "of", "to", "pay", "number", "cafe", "resume", "12", "50", "no"]      # one piece each


def _texts(n=40):
    rng = np.random.default_rng(7)
    counts = [1, 2, 6, 7, 14, 15, 30, 60, 126] + [int(c) for c in rng.integers(1, 40, n - 9)]
    return [" ".join(WORDS[j] for j in rng.integers(0, len(WORDS), c)) for c in counts]


@pytest.fixture(scope="module")
def tok(golden):
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    return WordPieceTokenizer(golden[1]["vocab"])


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_embed_texts_equals_the_single_texts_in_input_order(ctx, emb_mod, golden, tok, precision):
    state, _, _ = _case(golden, "A")
    e = emb_mod.JinaEmbeddings(state=state, config=R.config_json(R.CONFIG_A), tokenizer=tok, precision=precision, ctx=ctx)
    try:
        texts = _texts()
        whole = e.embed_texts(texts, chunk=16)
        calls = e.text_encoder_calls
        assert whole.shape == (40, 64) and whole.dtype == np.float32 and 3 <= calls <= 12 and e.texts_embedded == 40
        for i, text in enumerate(texts):
            assert np.array_equal(e.embed_texts([text])[0], whole[i]), f"text {i}"
        assert np.array_equal(e.embed_texts(texts), whole)           # and of the chunking
        ids, lens = tok.pad(e.encode_texts(texts), 128)
        print(f"embed_texts {precision}: 40 texts of {min(lens)} .. {max(lens)} tokens in {calls} calls")
        assert min(lens) == 3 and max(lens) == 128
        if precision == "f32":      # against the restatement (f16: test_f16_within_twice_the_emulated_rounding_error)
            err = np.abs(whole - R.forward(state, R.CONFIG_A, ids, lens)[1]).max()
            print(f"embed_texts f32: max |d| {err:.3e}")
            assert err <= 1e-3
        with pytest.raises(ValueError, match="too long"):
            e.embed_texts([" ".join(["invoice"] * 127)])
        cut = e.embed_texts([" ".join(["invoice"] * 127)], truncation=True)
        assert np.array_equal(cut, e.embed_texts([" ".join(["invoice"] * 126)]))
        out = e.get_embeddings(texts[:3])
        assert np.array_equal(out.embeddings, whole[:3]) and out.total_tokens == -1
    finally:
        e.close()


def test_meta_template_matcher_takes_sentence_embeddings(ctx, emb_mod, golden, tok, tmp_path):
    import json

    from safetensors.numpy import save_file

    from marie_icr_amd.template_matching import MetaTemplateMatcher

    # a model directory as sentence-transformers writes it
    state, _, _ = _case(golden, "B")
    d = str(tmp_path)
    save_file({"bert." + k: v for k, v in state.items()}, os.path.join(d, "model.safetensors"))
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(R.config_json(R.CONFIG_B), f)
    with open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(golden[1]["vocab"]) + "\n")
    e = emb_mod.SentenceTransformerEmbeddings(d, precision="f32", ctx=ctx)
    try:
        assert (e.pooling, e.normalize, e.max_seq_length, e.max_tokens) == ("mean", True, 128, 128)
        matcher = MetaTemplateMatcher(embeddings_processor=lambda clip: np.ones(4), text_embeddings_processor=e, ctx=ctx)
        pairs = [("INVOICE TOTAL", "INVOICE TOTAL"), ("TOTAL DUE", "INVOICE TOTAL"), ("PAYMENT DATE", "INVOICE TOTAL"),
                 ("AMOUNT DUE", "TOTAL DUE"), ("THE NUMBER OF THE INVOICE " * 30, "INVOICE NUMBER")]
        sims = matcher.text_sims(pairs)
        texts = list(dict.fromkeys(t for p in pairs for t in p))
        ids, lens = tok.pad([tok.encode(t[:1024], 128) for t in texts], 128)
        _, ref = R.forward(state, R.CONFIG_B, ids, lens, "mean", True)
        cos = R.cosine_matrix(ref)
        want = [cos[texts.index(a), texts.index(b)] for a, b in pairs]
        err = np.abs(np.array(sims) - np.array(want)).max()
        print(f"MetaTemplateMatcher.text_sims: {np.round(sims, 4)}, max |d cosine| {err:.3e}")
        assert sims[0] == 1.0 and err <= 1e-5 and max(lens) == 128
        out = e.get_embeddings(["invoice total", "the"])
        assert out.embeddings.shape == (2, 128) and out.total_tokens == 128
        assert np.allclose(np.sqrt((out.embeddings.astype(np.float64) ** 2).sum(-1)), 1.0, atol=1e-6)
        cosines, emb = e.text_cosine_pairs(["total", "invoice", "total"], [(0, 1), (0, 2)], want_embeddings=True)
        assert cosines[1] == 1.0 and np.array_equal(emb[0], emb[2]) and abs(cosines[0]) < 0.999
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_create_and_calls_refuse_what_the_kernels_do_not_cover(ctx, emb_mod, golden):
    from marie_icr_amd._lib import BertTextConfig, MarieHipError

    good = dict(vocab=80, max_position=128, type_vocab=2, dim=128, heads=2, depth=2, ffn=256, ln_eps=1e-12, position=0, mlp=0, pool=0,
                normalize=0)
    for change, field in ((dict(dim=96, heads=2), "dim"), (dict(dim=192, heads=4), "head"), (dict(heads=3), "heads"), (dict(dim=2048, heads=32), "dim"),
                          (dict(ffn=100), "ffn"), (dict(position=2), "position"), (dict(mlp=2), "mlp"), (dict(pool=2), "pool"),
                          (dict(normalize=2), "normalize")):
        with pytest.raises(MarieHipError, match=field):
            emb_mod.BertTextModel(ctx, None, BertTextConfig(**dict(good, **change)), F32)
    m = _model(ctx, emb_mod, golden, "B", F32)
    _, ids, lens = _case(golden, "B")
    ctx.profile_enable(True)
    ctx.profile_reset()

    def refused(i, n):
        with pytest.raises(MarieHipError):
            m.embed_ids_host(i, n)

    refused(np.zeros((4, 12), np.int32), np.ones(4, np.int32))      # rows no multiple of 8
    refused(np.zeros((4, 136), np.int32), np.ones(4, np.int32))     # more rows than the kernel holds
    for bad in (0, 25, -1):
        changed = lens.copy()
        changed[2] = bad
        refused(ids, changed)
    for bad in (-1, 80):
        changed = ids.copy()
        changed[1, 23] = bad                                       # a padding row's id counts too
        refused(changed, lens)
    refused(np.zeros((4097, 8), np.int32), np.ones(4097, np.int32))
    with pytest.raises(MarieHipError):
        m.embed_pairs_host(ids, lens, [(0, 4)])
    q = np.zeros((1, 8, 96), np.float32)
    with pytest.raises(MarieHipError, match="head_dim 48"):
        emb_mod.short_attention_host(ctx, F32, q, q, q, [8], 2)
    with pytest.raises(MarieHipError):
        emb_mod.short_attention_host(ctx, F32, q[:, :, :64], q[:, :, :64], q[:, :, :64], [9], 2)
    unfinished = emb_mod.BertTextModel(ctx, None, BertTextConfig(**good), F32)
    with pytest.raises(MarieHipError):
        unfinished.embed_ids_host(ids, lens)
    unfinished.close()
    # a state with a tensor missing: finalize names it
    state, _, _ = _case(golden, "B")
    tensors, cfg = emb_mod.load_bert_text_state(state, R.config_json(R.CONFIG_B))
    del tensors["encoder.layer.1.output.LayerNorm.bias"]
    with pytest.raises(MarieHipError, match=r"encoder\.layer\.1\.output\.LayerNorm\.bias"):
        emb_mod.BertTextModel(ctx, tensors, cfg, F32)
    # all of that before any launch
    after = ctx.profile_read()
    ctx.profile_enable(False)
    assert all(after[k]["launches"] == 0 for k in after), {k: v["launches"] for k, v in after.items() if v["launches"]}
    assert m.embed_ids_host(ids, lens).shape == (4, 128)
