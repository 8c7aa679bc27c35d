"""BERT sentence embeddings past 128 tokens on the MI355X: the streamed attention attn_long (marie_icr_amd/csrc/attn_seq.hip)
alone, the encoders at npad 512 and the public classes, against tests/bert_text_ref.py — the float64 restatement that
tests/test_berttext_long_cpu.py pins to transformers.BertModel at these lengths through tests/golden/bert_text_long.npz.

Bars, those of tests/test_berttext_gpu.py:
  * fp32: 1e-3 absolute on O(1) quantities for the kernel, stream taps and embeddings, 1e-5 for cosines;
  * f16: E_ref = max |f16-rounded restatement - float64 restatement| is computed here on the CPU for each case, and
    max |kernel - float64 restatement| <= 2 E_ref.  The emulation rounds the probabilities against the row's maximum, the kernel
    against the running one: a relative rounding does not care about the scale;
  * a text's rows do not depend on npad, on its batch or on what lies past its length: bitwise, in both precisions.
Every test prints its figures before it asserts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_long as RL  # noqa: E402
import bert_text_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHORT_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_text.npz")
F32, F16 = 1, 0
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
    return RL.load_long_golden()


@pytest.fixture(scope="module")
def tok():
    from marie_icr_amd.wordpiece_tokenizer import WordPieceTokenizer

    return WordPieceTokenizer(R.load_golden(SHORT_GOLDEN)[1]["vocab"])


def _qkv(npad, hd, B=6, heads=2):
    """the input recipe of tests/test_berttext_gpu.py: three different draws, a ramp over the position on k and over the head dim
    on v"""
    rng = np.random.default_rng(1000 * hd + npad)
    D = heads * hd
    q = rng.standard_normal((B, npad, D)) * (R.LOG2E / np.sqrt(hd))
    k = rng.standard_normal((B, npad, D)) + 0.3 * np.linspace(-1, 1, npad)[None, :, None]
    v = rng.standard_normal((B, npad, D)) + np.linspace(-1, 1, D)[None, None, :]
    return [np.ascontiguousarray(a, np.float32) for a in (q, k, v)]


SLOPES = np.array([0.5, 0.0625]) * R.LOG2E      # log2 units, as the encoder passes them
HEADS = 2

# (npad, lens): a second block of one tile, whose f16 32-key step takes a zero tile; the block edge, one full tile, tile + 1; a
# third block; nine blocks of rescaling; a single block through the streamed code
SHAPES = [(136, (1, 17, 128, 129, 136)), (256, (129, 144, 145, 255, 256)), (264, (257, 264)), (1040, (1025, 1040)), (128, (7, 128))]


def _computed(lens, npad):
    """bool (B, npad): the rows attn_long computes — those of the 64-query blocks that start below the length, queries past the
    length inside such a block included; the blocks past it are written as zeros (section 3)"""
    return np.arange(npad)[None, :] < (np.asarray(lens)[:, None] + 63) // 64 * 64


def _kernel_case(npad, lens, hd, alibi, f16):
    """(q, k, v, lens, float64 reference or its f16 emulation), computed once and left unchanged"""
    key = ("attn", npad, hd, alibi, f16)
    if key not in _cache:
        q, k, v = _qkv(npad, hd, B=len(lens))
        slopes = SLOPES if alibi else None
        if f16:
            out = R.r16(R.attention(R.r16(q), R.r16(k), R.r16(v), lens, HEADS, slopes, f16=True))
        else:
            out = R.attention(*(a.astype(np.float64) for a in (q, k, v)), lens, HEADS, slopes)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- 1. attn_long alone
# first MI355X run: f32 6.7e-7 .. 2.7e-6 (largest: npad 1040 with ALiBi); f16 max |kernel - fp64| 5.63e-4 .. 2.60e-3 over the twenty
# cases, equal to E_ref of its case to the four digits printed in nineteen and below it in one (hd 64, npad 264, plain: 6.21e-4
# against 6.42e-4); 8192 rows: f32 2.8e-6, f16 1.264e-3 (E_ref 1.264e-3).  No streamed-rounding emulation was needed
@pytest.mark.parametrize("alibi", [False, True], ids=["plain", "alibi"])
@pytest.mark.parametrize("npad,lens", SHAPES, ids=[f"npad{n}" for n, _ in SHAPES])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_long_kernel(ctx, emb_mod, precision, hd, npad, lens, alibi):
    lens = np.array(lens, np.int32)
    q, k, v = _qkv(npad, hd, B=len(lens))
    slopes = SLOPES if alibi else None
    want = _kernel_case(npad, lens, hd, alibi, False)
    got = emb_mod.long_attention_host(ctx, precision, q, k, v, lens, HEADS, slopes)
    rows = _computed(lens, npad)
    err = np.abs(got - want)[rows].max()
    what = f"hd {hd} npad {npad} {'alibi' if alibi else 'plain'}"
    if precision == F32:
        print(f"attn_long f32 {what}: max |d| {err:.3e} (outputs up to {np.abs(want[rows]).max():.2f})")
    else:
        e_ref = np.abs(_kernel_case(npad, lens, hd, alibi, True) - want)[rows].max()
        print(f"attn_long f16 {what}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    assert 0.5 <= np.abs(want[rows]).max() <= 8 and np.isfinite(got).all()
    assert err <= (1e-3 if precision == F32 else 2 * e_ref)
    assert (got[~rows] == 0).all()


def _blocked_case(f16):
    key = ("full", f16)
    if key not in _cache:
        npad, n = 8192, 8185
        q, k, v = _qkv(npad, 64, B=1, heads=1)
        if f16:
            out = R.r16(RL.attention_blocked(R.r16(q[0]), R.r16(k[0]), R.r16(v[0]), n, SLOPES[1], True))
        else:
            out = RL.attention_blocked(*(a[0].astype(np.float64) for a in (q, k, v)), n, SLOPES[1])
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- 2. the full length
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_long_at_8192_rows(ctx, emb_mod, precision):
    npad, n = 8192, 8185
    q, k, v = _qkv(npad, 64, B=1, heads=1)
    want = _blocked_case(False)
    got = emb_mod.long_attention_host(ctx, precision, q, k, v, [n], 1, SLOPES[1:])[0]
    err = np.abs(got - want).max()
    if precision == F32:
        print(f"attn_long f32 npad 8192 len 8185 alibi: max |d| {err:.3e} (outputs up to {np.abs(want).max():.2f})")
    else:
        e_ref = np.abs(_blocked_case(True) - want).max()
        print(f"attn_long f16 npad 8192 len 8185 alibi: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    assert 0.5 <= np.abs(want).max() <= 8 and np.isfinite(got).all()
    assert err <= (1e-3 if precision == F32 else 2 * e_ref)


def _state(golden, name):
    if name == "B_jina":
        if ("state", name) not in _cache:
            _cache[("state", name)] = R.quantize_state(R.make_state(RL.CONFIG_B_JINA, 13))[0]
        return _cache[("state", name)], golden["B"]["ids"], golden["B"]["lens"]
    g = golden[name]
    return g["state"], g["ids"], g["lens"]


def _model(ctx, emb_mod, golden, name, precision, mode="mean", normalize=False):
    key = ("model", name, precision, mode, normalize)
    if key not in _cache:
        tensors, cfg = emb_mod.load_bert_text_state(_state(golden, name)[0], R.config_json(RL.CONFIGS[name]))
        cfg.pool, cfg.normalize = (emb_mod.POOL_CLS if mode == "cls" else emb_mod.POOL_MEAN), int(normalize)
        _cache[key] = emb_mod.BertTextModel(ctx, tensors, cfg, precision)
    return _cache[key]


def test_rows_past_the_limits_are_refused_before_any_launch(ctx, emb_mod, golden):
    from marie_icr_amd._lib import MarieHipError

    jina, plain = _model(ctx, emb_mod, golden, "B_jina", F32), _model(ctx, emb_mod, golden, "A", F32)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for m, shape in ((jina, (1, 8200)), (jina, (4097, 136)), (jina, (4096, 136)), (plain, (1, 520)), (plain, (4096, 136))):
        with pytest.raises(MarieHipError):
            m.embed_ids_host(np.zeros(shape, np.int32), np.ones(shape[0], np.int32))
        assert m.workspace_bytes(*shape) == 0
    x = np.zeros((1, 8200, 64), np.float32)
    with pytest.raises(MarieHipError):
        emb_mod.long_attention_host(ctx, F32, x, x, x, [8200], 1)
    with pytest.raises(MarieHipError):                                 # the LDS-resident entry keeps its limit
        emb_mod.short_attention_host(ctx, F32, x[:, :136], x[:, :136], x[:, :136], [136], 1)
    with pytest.raises(MarieHipError, match="head_dim 48"):
        emb_mod.long_attention_host(ctx, F32, x[:, :136, :48], x[:, :136, :48], x[:, :136, :48], [136], 1)
    after = ctx.profile_read()
    ctx.profile_enable(False)
    assert all(after[k]["launches"] == 0 for k in after), {k: v["launches"] for k, v in after.items() if v["launches"]}
    assert jina.workspace_bytes(3855, 136) > 0 and jina.workspace_bytes(64, 8192) > 0


# ---------------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("alibi", [False, True], ids=["plain", "alibi"])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_long_rows_depend_on_the_sequence_alone_bitwise(ctx, emb_mod, precision, alibi):
    hd, npad = 32, 264
    slopes = SLOPES if alibi else None
    lens = np.array([1, 129, 200, 257, 64, 264], np.int32)
    q, k, v = _qkv(npad, hd)
    got = emb_mod.long_attention_host(ctx, precision, q, k, v, lens, HEADS, slopes)
    assert np.isfinite(got).all()
    # what lies past a sequence's length does not reach it, queries past the length included
    k2, v2 = k.copy(), v.copy()
    for b, n in enumerate(lens):
        k2[b, n:] = k2[b, n:] * -1.5 + 2.0
        v2[b, n:] += 3.0
    assert np.array_equal(emb_mod.long_attention_host(ctx, precision, q, k2, v2, lens, HEADS, slopes), got)
    # the text of 200 tokens: alone at npad 200, in the batch of six at 264, alone at 1040
    b, n = 2, 200
    alone = emb_mod.long_attention_host(ctx, precision, q[b:b + 1, :n], k[b:b + 1, :n], v[b:b + 1, :n], [n], HEADS, slopes)
    assert np.array_equal(alone[0], got[b, :n])
    wide = [np.ascontiguousarray(np.concatenate([a[b:b + 1], _qkv(1040 - npad, hd, B=1)[i]], 1)) for i, a in enumerate((q, k, v))]
    far = emb_mod.long_attention_host(ctx, precision, *wide, [n], HEADS, slopes)
    assert np.array_equal(far[0, :n], got[b, :n])
    # query blocks (of 64) wholly past the length are written as zeros; a block that starts below it is computed
    for b, n in enumerate(lens):
        first = min((int(n) + 63) // 64 * 64, npad)
        assert (got[b, first:] == 0).all() and (first == int(n) or np.abs(got[b, n:first]).min() > 0)
    assert (far[0, 256:] == 0).all() and np.abs(far[0, 200:256]).min() > 0
    # a sequence of one key returns that key's values
    want0 = v[0, 0] if precision == F32 else v[0, 0].astype(np.float16).astype(np.float32)
    assert np.array_equal(got[0, :64], np.broadcast_to(want0, got[0, :64].shape))


# ---------------------------------------------------------------------------------------------------- 4. rescale order
@pytest.mark.parametrize("first", [96, 186], ids=["keys96-159", "keys186-249"])
def test_attn_long_probabilities_across_a_block_edge(ctx, emb_mod, first):
    """exact data: q = 0, so the scores are the bias alone, and one-hot values read the probabilities of 64 keys back.  For the
    queries left of the window the maximum sits in block 0 and alpha = 1 afterwards; for those right of it the maximum moves up
    block by block"""
    npad, hd, n = 264, 64, 250
    q = np.zeros((1, npad, HEADS * hd), np.float32)
    k = np.ones_like(q)
    v = np.zeros_like(q)
    for h in range(HEADS):
        v[0, first + np.arange(hd), h * hd + np.arange(hd)] = 1.0       # value d of key first + d is 1
    got = emb_mod.long_attention_host(ctx, F32, q, k, v, [n], HEADS, SLOPES)
    i, j = np.meshgrid(np.arange(npad), np.arange(n), indexing="ij")
    for h in range(HEADS):
        p = got[0, :, h * hd:(h + 1) * hd].astype(np.float64)           # p[i, d] = probability of key first + d
        full = np.exp2(-SLOPES[h] * np.abs(i - j))
        want = full[:, first:first + hd] / full.sum(-1, keepdims=True)
        err = np.abs(p[:256] - want[:256]).max()
        print(f"attn_long probabilities of keys {first} .. {first + hd - 1}, head {h}: max |d| {err:.3e} (largest {want.max():.3f})")
        assert err <= 1e-6
        assert (p[256:] == 0).all()                                      # the query block at 256 starts past the 250 keys


# ---------------------------------------------------------------------------------------------------- 5. the encoders at npad 512
def _reference(golden, name, mode="mean", normalize=False, f16=False):
    key = ("ref", name, mode, normalize, f16)
    if key not in _cache:
        state, ids, lens = _state(golden, name)
        taps, emb = R.forward(state, RL.CONFIGS[name], ids, lens, mode, normalize, f16)
        taps.setflags(write=False)
        emb.setflags(write=False)
        _cache[key] = (taps, emb)
    return _cache[key]


def _all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


@pytest.mark.parametrize("name", ["A", "B", "B_jina"])
def test_fp32_encoder_at_512_rows(ctx, emb_mod, golden, name):
    _, ids, lens = _state(golden, name)
    valid = R.valid_rows(lens, ids.shape[1])
    ref_taps, _ = _reference(golden, name)
    assert 0.5 <= np.abs(ref_taps[:, valid]).max() <= 10
    m = _model(ctx, emb_mod, golden, name, F32)
    taps, emb = m.debug_taps_host(ids, lens)
    assert np.isfinite(taps).all()
    tap_err = [float(np.abs(taps[i] - ref_taps[i])[valid].max()) for i in range(len(taps))]
    print(f"{name} fp32 npad 512: taps {' '.join(f'{e:.2e}' for e in tap_err)}")
    for i, e in enumerate(tap_err):
        assert e <= 1e-3, f"tap {i} (0: the embedding kernel, k: layer k)"
    for mode, norm, stored in (("mean", False, "mean"), ("mean", True, "mean_norm"), ("cls", False, "cls")):
        ref_emb = _reference(golden, name, mode, norm)[1]
        mm = _model(ctx, emb_mod, golden, name, F32, mode, norm)
        cos, got = mm.embed_pairs_host(ids, lens, _all_pairs(len(ids)), want_embeddings=True)
        ref_cos = R.cosine_matrix(ref_emb)
        emb_err, cos_err = np.abs(got - ref_emb).max(), np.abs(cos.reshape(ref_cos.shape) - ref_cos).max()
        line = f"{name} fp32 npad 512 {mode}{' normalized' if norm else ''}: embeddings {emb_err:.3e}; cosines {cos_err:.3e}"
        if name != "B_jina":      # what transformers computed
            hf_err = np.abs(got - golden[name][stored]).max()
            line += f"; against transformers {hf_err:.3e}"
        print(line)
        assert emb_err <= 1e-3 and cos_err <= 1e-5
        assert name == "B_jina" or hf_err <= 1e-3
        assert np.array_equal(got, mm.embed_ids_host(ids, lens))
        if (mode, norm) == ("mean", False):
            assert np.array_equal(got, emb)
    if name != "B_jina":
        rows_err = np.abs(RL.take_rows(taps, golden[name]["rows"]) - golden[name]["hidden_rows"]).max()
        print(f"{name} fp32 npad 512: the golden's hidden rows {rows_err:.3e}")
        assert rows_err <= 1e-3


@pytest.mark.parametrize("name", ["A", "B", "B_jina"])
def test_f16_encoder_at_512_rows_within_twice_the_emulated_rounding_error(ctx, emb_mod, golden, name):
    _, ids, lens = _state(golden, name)
    valid = R.valid_rows(lens, ids.shape[1])
    ref_taps, ref_emb = _reference(golden, name)
    emu_taps, emu_emb = _reference(golden, name, f16=True)
    m = _model(ctx, emb_mod, golden, name, F16)
    taps, emb = m.debug_taps_host(ids, lens)
    assert np.isfinite(taps).all()
    checks = []
    for i in range(len(taps)):
        err, e_ref = np.abs(taps[i] - ref_taps[i])[valid].max(), np.abs(emu_taps[i] - ref_taps[i])[valid].max()
        print(f"{name} f16 npad 512 tap {i}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        checks.append((f"tap {i}", err, 1e-3 if i == 0 else 2 * e_ref))      # nothing is rounded to f16 before the first GEMM
    err, e_ref = np.abs(emb - ref_emb).max(), np.abs(emu_emb - ref_emb).max()
    print(f"{name} f16 npad 512 embeddings: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    checks.append(("embeddings", err, 2 * e_ref))
    cos = m.embed_pairs_host(ids, lens, _all_pairs(len(ids))).reshape(len(ids), len(ids))
    ref_cos, emu_cos = R.cosine_matrix(ref_emb), R.cosine_matrix(emu_emb)
    err, e_ref = np.abs(cos - ref_cos).max(), np.abs(emu_cos - ref_cos).max()
    print(f"{name} f16 npad 512 cosines: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    checks.append(("cosines", err, 2 * e_ref))
    for what, err, bar in checks:
        assert err <= bar, what


# ---------------------------------------------------------------------------------------------------- 6. the public classes
WORDS = ["the", "invoice", "total", "amount", "due", "date", "of", "to", "pay", "number", "cafe", "resume", "12", "50", "no"]      # one piece each


def _words(rng, count):
    return " ".join(WORDS[j] for j in rng.integers(0, len(WORDS), count))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_embed_texts_across_the_boundary_equals_the_single_texts(ctx, emb_mod, golden, tok, precision):
    state = golden["A"]["state"]
    conf = R.config_json(RL.CONFIG_A)
    e = emb_mod.SentenceTransformerEmbeddings(state=state, config=conf, tokenizer=tok, precision=precision, ctx=ctx)
    assert (e.max_seq_length, e.max_tokens) == (256, 256)
    e.close()
    e = emb_mod.SentenceTransformerEmbeddings(state=state, config=conf, tokenizer=tok, precision=precision, ctx=ctx, max_seq_length=512)
    try:
        assert (e.max_seq_length, e.max_tokens) == (512, 512)
        rng = np.random.default_rng(11)
        assert e.embed_texts([_words(rng, 300)]).shape == (1, 64)      # 302 tokens, no truncation
        tokens = [3, 4, 60, 127, 128, 129, 130, 136, 137, 256, 257, 384, 385, 499, 500] + [int(c) for c in rng.integers(3, 501, 15)]
        texts = [_words(rng, c - 2) for c in tokens]
        lengths = [len(ids) for ids in e.encode_texts(texts)]
        assert lengths == tokens
        groups = e._groups(lengths, 8)
        for npad, members in groups:
            own = [lengths[i] for i in members]
            assert (max(own) <= 128 or min(own) > 128) and (npad <= 128) == (max(own) <= 128) and len(members) <= 8
        before = e.text_encoder_calls
        whole = e.embed_texts(texts, chunk=8)
        assert e.text_encoder_calls - before == len(groups) and whole.shape == (30, 64) and np.isfinite(whole).all()
        for i, text in enumerate(texts):
            assert np.array_equal(e.embed_texts([text])[0], whole[i]), f"text {i} of {tokens[i]} tokens depends on its batch"
        assert np.array_equal(e.embed_texts(texts), whole)             # and of the chunking
        print(f"embed_texts {precision}: 30 texts of {min(tokens)} .. {max(tokens)} tokens in {len(groups)} calls of "
              f"{[npad for npad, _ in groups]} rows: equal bits alone")
        if precision == "f32":
            ids, lens = tok.pad(e.encode_texts(texts), 504)
            err = np.abs(whole - R.forward(state, RL.CONFIG_A, ids, lens, "mean", True)[1]).max()
            print(f"embed_texts f32: max |d| {err:.3e}")
            assert err <= 1e-3
        with pytest.raises(ValueError, match="too long: 513 tokens"):
            e.embed_texts([_words(rng, 511)])
    finally:
        e.close()


def test_jina_shaped_class_takes_8192_tokens(ctx, emb_mod, golden, tok):
    state = _state(golden, "B_jina")[0]
    e = emb_mod.JinaEmbeddings(state=state, config=R.config_json(RL.CONFIG_B_JINA), tokenizer=tok, precision="f16", ctx=ctx)
    try:
        assert e.max_seq_length is None and e.max_tokens == 8192
        text = " ".join(["invoice"] * 8191)                              # 8193 tokens
        with pytest.raises(ValueError, match="too long: 8193 tokens"):
            e.encode_texts([text])
        cut = e.encode_texts([text], truncation=True)[0]
        assert len(cut) == 8192 and cut[0] == tok.cls_id and cut[-1] == tok.sep_id
        out = e.embed_texts([" ".join(["invoice"] * 298), "total due"])
        assert out.shape == (2, 128) and np.isfinite(out).all()
    finally:
        e.close()
