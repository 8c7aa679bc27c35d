"""CLIP text tower on the MI355X (marie_icr_amd/csrc/cliptext_api.hip, cliptext_ops.hip, attn_seq.hip) against tests/cliptext_ref.py, the
plain-torch restatement that tests/test_cliptext_cpu.py pins to transformers.CLIPTextModelWithProjection in float64.

Bars (the project's own, as tests/test_clip_gpu.py sets them):
  * the kernels alone against fp64: 1e-3 absolute on O(1) quantities; the causal attention in f16 mode against fp64 on the
    f16-rounded inputs: 2 x a constant measured on the MI355X (one seed, hence the factor);
  * fp32 mode against the fp32 restatement: residual-stream taps and embeddings 1e-3, cosines 1e-5;
  * f16 mode against the fp32 restatement: 2 x constants measured on the MI355X, and the order of two reference cosines wherever
    their gap exceeds twice the cosine bar (at most a quarter of the pairs of cosines may be closer than that);
  * a text's embedding does not depend on the call it is part of: bitwise.
Every test prints its figures before it asserts.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as V  # noqa: E402
import cliptext_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# attn_causal alone, f16 mode, against fp64 on the f16-rounded inputs: max over B 3 x heads 2 x npad {8, 16, 24, 40, 72, 80}
# (first MI355X run: 1.121e-3, 1.148e-3, 1.074e-3, 1.063e-3, 1.129e-3, 9.78e-4 in that order, outputs up to 4.6: the output's own
# f16 rounding is up to 9.8e-4 of it; fp32 mode on the same inputs: 9.3e-7).  npad 104 and 128, added when the kernel moved to
# attn_seq.hip, outputs up to 3.37: 9.972e-4 and 1.228e-3 with the kernel before the move and, bit for bit, with the one after it
# (fp32 mode 8.6e-7 and 1.13e-6); the constant is the first run's and was not raised
F16_ATTN_CAUSAL_ERR_MEASURED = 1.148e-3
# f16 tower against the fp32 restatement, max over SMALL on the nine texts and ViT-B/32 text geometry on the eight id sequences
# (first MI355X run: small 9.09e-4 / 1.027e-4, ViT-B/32 text 4.424e-3 / 1.949e-4; fp32 mode: 8.3e-7 / 1.9e-7 and 7.3e-6 / 1.2e-7)
F16_CLIPTEXT_EMBED_ERR_MEASURED = 4.424e-3   # max |d embedding entry| (entries up to 3.7)
F16_CLIPTEXT_COS_ERR_MEASURED = 1.949e-4     # max |d cosine| over all pairs of a case's texts

SCORE_SCALE = 0.125 * 1.4426950408889634      # head_dim^-0.5 * log2(e): the units attn_causal takes q in
CASES = {"small": R.SMALL, "vit_b32_text": R.VIT_B32_TEXT}
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
def vocab_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cliptext"))
    R.make_vocab(d)
    return d


@pytest.fixture(scope="module")
def tok(vocab_dir):
    from marie_icr_amd.clip_tokenizer import ClipTokenizer

    return ClipTokenizer.from_dir(vocab_dir)


def _state(name):
    if ("state", name) not in _cache:
        _cache[("state", name)] = R.make_state(CASES[name], seed=0)
    return _cache[("state", name)]


def _ids(name, tok):
    return tok.encode_batch(R.TEXTS) if name == "small" else R.random_ids(R.VIT_B32_TEXT)


def _reference(name, tok):
    """(ids, eot, taps, embeddings, cosine matrix) of a case from the fp32 restatement, computed once"""
    if ("ref", name) not in _cache:
        ids, eot = _ids(name, tok)
        taps, emb = R.forward(_state(name), CASES[name], ids, eot, torch.float32)
        taps, emb = taps.numpy(), emb.numpy()
        cos = R.cosine_matrix(torch.from_numpy(emb).double()).numpy()
        off = cos[~np.eye(len(cos), dtype=bool)]
        print(f"{name}: reference cosines {off.min():.3f} .. {off.max():.3f}, largest embedding entry {np.abs(emb).max():.2f}, "
              f"largest stream entry {np.abs(taps).max():.1f}")
        assert off.min() < 0.7 and off.max() > 0.99, "the texts are not told apart"
        assert 0.5 <= np.abs(emb).max() <= 10
        for a in (ids, eot, taps, emb, cos):
            a.setflags(write=False)
        _cache[("ref", name)] = (ids, eot, taps, emb, cos)
    return _cache[("ref", name)]


def _model(ctx, emb_mod, name, precision):
    if ("model", name, precision) not in _cache:
        tensors, cfg = emb_mod.load_clip_text_state(_state(name))
        _cache[("model", name, precision)] = emb_mod.ClipTextModel(ctx, tensors, cfg, precision)
    return _cache[("model", name, precision)]


def _all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


# ---------------------------------------------------------------------------------------------------- 1. attn_causal alone
def _qkv(npad, B=3, heads=2):
    """asymmetric O(1) inputs: three different draws, and a ramp over the head dim on v and over the position on k"""
    rng = np.random.default_rng(100 + npad)
    D = heads * 64
    q = rng.standard_normal((B, npad, D)) * SCORE_SCALE
    k = rng.standard_normal((B, npad, D)) + 0.3 * np.linspace(-1, 1, npad)[None, :, None]
    v = rng.standard_normal((B, npad, D)) + np.linspace(-1, 1, D)[None, None, :]
    return [np.ascontiguousarray(a, np.float32) for a in (q, k, v)]


# the sizes cross the 16-query tile, the 32-key MFMA step, the 64-key tile and the maximum of the 77-token context; at 104 and 128
# a wave's second query tile walks six to eight key tiles, and 128 is the kernel's row limit
@pytest.mark.parametrize("npad", [8, 16, 24, 40, 72, 80, 104, 128])
@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
def test_attn_causal_kernel(ctx, emb_mod, precision, npad):
    heads = 2
    q, k, v = _qkv(npad)
    if precision == 0:      # the kernel sees the f16 roundings; the reference is given the same
        q, k, v = (a.astype(np.float16).astype(np.float32) for a in (q, k, v))
    got = emb_mod.causal_attention_host(ctx, precision, q, k, v, heads)
    want = R.causal_attention_fp64(q, k, v, heads)
    err = np.abs(got - want).max()
    print(f"attn_causal {'f32' if precision else 'f16'} npad {npad}: max |d| {err:.3e} (outputs up to {np.abs(want).max():.2f}; "
          f"f16 constant {F16_ATTN_CAUSAL_ERR_MEASURED})")
    assert 0.5 <= np.abs(want).max() <= 8
    assert np.isfinite(got).all()
    if precision == 1:
        assert err <= 1e-3
    else:
        assert F16_ATTN_CAUSAL_ERR_MEASURED is not None, "the f16 causal attention error has not been measured on an MI355X yet"
        assert err <= 2 * F16_ATTN_CAUSAL_ERR_MEASURED
    # row 0 sees key 0 alone
    assert np.array_equal(got[:, 0], v[:, 0])
    # what follows row t does not reach it: bitwise
    for t in sorted({0, 5, 15, 16, npad // 2, npad - 2}):
        if t >= npad - 1:
            continue
        k2, v2 = k.copy(), v.copy()
        k2[:, t + 1:] = k2[:, t + 1:] * -1.5 + 2.0
        v2[:, t + 1:] += 3.0
        other = emb_mod.causal_attention_host(ctx, precision, q, k2, v2, heads)
        assert np.array_equal(other[:, :t + 1], got[:, :t + 1]), f"row <= {t} changed with the keys after it"
        assert not np.array_equal(other[:, t + 1], got[:, t + 1])


# ---------------------------------------------------------------------------------------------------- 2. embedding and head alone
@pytest.mark.parametrize("B,npad,D,vocab", [(3, 8, 128, 50), (5, 80, 512, 300), (2, 24, 1024, 7)])
def test_embed_kernel(ctx, emb_mod, B, npad, D, vocab):
    rng = np.random.default_rng(B * D)
    table, pos = rng.standard_normal((vocab, D)).astype(np.float32), rng.standard_normal((npad, D)).astype(np.float32)
    ids = rng.integers(0, vocab, (B, npad)).astype(np.int32)
    ids[0, 0], ids[0, 1], ids[-1, -1], ids[-1, 0] = 0, vocab - 1, vocab - 1, 0
    got = emb_mod.text_embed_rows_host(ctx, table, pos, ids)
    want = table.astype(np.float64)[ids] + pos.astype(np.float64)
    err = np.abs(got - want).max()
    print(f"cliptext_embed B {B} npad {npad} D {D}: max |d| {err:.3e}")
    assert err <= 1e-3
    assert np.array_equal(got, table[ids] + pos)            # one fp32 addition an entry


@pytest.mark.parametrize("B,npad,D,E", [(3, 8, 128, 64), (4, 80, 512, 512), (2, 16, 1024, 100)])
def test_head_kernel_with_row_of(ctx, emb_mod, B, npad, D, E):
    rng = np.random.default_rng(B + D + E)
    h = rng.standard_normal((B, npad, D)).astype(np.float32) * 2 + 0.5
    g, b = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)
    proj = (rng.standard_normal((D, E)) / np.sqrt(D)).astype(np.float32)
    rows = rng.integers(1, npad, B).astype(np.int32)
    rows[0], rows[-1] = 1, npad - 1
    got = emb_mod.text_head_host(ctx, h, g, b, proj, rows)
    x = h.astype(np.float64)[np.arange(B), rows]
    want = ((x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5) * g + b) @ proj.astype(np.float64)
    err = np.abs(got - want).max()
    print(f"head B {B} npad {npad} D {D} E {E}: max |d| {err:.3e} (entries up to {np.abs(want).max():.2f})")
    assert err <= 1e-3
    # row 0 of every block is what the vision head takes: the same launcher without row_of
    zero = emb_mod.text_head_host(ctx, h, g, b, proj, np.zeros(B, np.int32))
    assert np.array_equal(zero, emb_mod.head_host(ctx, h, g, b, proj, 1e-5))


# ---------------------------------------------------------------------------------------------------- 3. fp32 tower
@pytest.mark.parametrize("name", ["small", "vit_b32_text"])
def test_fp32_taps_embeddings_and_cosines(ctx, emb_mod, tok, name):
    ids, eot, ref_taps, ref_emb, ref_cos = _reference(name, tok)
    m = _model(ctx, emb_mod, name, 1)
    taps, emb = m.debug_taps_host(ids, eot)
    pairs = _all_pairs(len(ids))
    cos, emb2 = m.embed_pairs_host(ids, eot, pairs, want_embeddings=True)
    cos = cos.reshape(ref_cos.shape)
    tap_err = [float(np.abs(taps[i] - ref_taps[i]).max()) for i in range(len(taps))]
    print(f"{name} fp32: taps {' '.join(f'{e:.2e}' for e in tap_err)}; embeddings {np.abs(emb - ref_emb).max():.3e}; "
          f"cosines {np.abs(cos - ref_cos).max():.3e}")
    for i, e in enumerate(tap_err):
        assert e <= 1e-3, f"tap {i} (0: the embedding kernel, k: layer k)"
    assert np.abs(emb - ref_emb).max() <= 1e-3
    assert np.abs(cos - ref_cos).max() <= 1e-5
    assert np.array_equal(emb, emb2) and np.array_equal(emb, m.embed_ids_host(ids, eot))
    assert m.workspace_bytes(len(ids), ids.shape[1]) > 0 and m.workspace_bytes(len(ids), ids.shape[1] + 1) == 0


# ---------------------------------------------------------------------------------------------------- 4. f16 tower
@pytest.mark.parametrize("name", ["small", "vit_b32_text"])
def test_f16_embeddings_and_cosines(ctx, emb_mod, tok, name):
    ids, eot, _, ref_emb, ref_cos = _reference(name, tok)
    m = _model(ctx, emb_mod, name, 0)
    cos, emb = m.embed_pairs_host(ids, eot, _all_pairs(len(ids)), want_embeddings=True)
    cos = cos.reshape(ref_cos.shape)
    emb_err, cos_err = np.abs(emb - ref_emb).max(), np.abs(cos - ref_cos).max()
    print(f"{name} f16: embeddings {emb_err:.3e} (entries up to {np.abs(ref_emb).max():.2f}); cosines {cos_err:.3e} "
          f"(measured constants {F16_CLIPTEXT_EMBED_ERR_MEASURED}, {F16_CLIPTEXT_COS_ERR_MEASURED})")
    assert F16_CLIPTEXT_EMBED_ERR_MEASURED is not None, "the f16 embedding error has not been measured on an MI355X yet"
    assert F16_CLIPTEXT_COS_ERR_MEASURED is not None, "the f16 cosine error has not been measured on an MI355X yet"
    emb_bound, cos_bound = 2 * F16_CLIPTEXT_EMBED_ERR_MEASURED, 2 * F16_CLIPTEXT_COS_ERR_MEASURED
    assert emb_err <= emb_bound and cos_err <= cos_bound
    # the order of two cosines the reference tells apart
    iu = np.triu_indices(len(ids), 1)
    r, g = ref_cos[iu], cos[iu]
    gap = r[:, None] - r[None, :]
    told = gap > 2 * cos_bound
    n_pairs = len(r) * (len(r) - 1) // 2
    aside = n_pairs - int(told.sum())
    print(f"{name} f16: {int(told.sum())} of {n_pairs} pairs of cosines are more than {2 * cos_bound:.2e} apart ({aside} set aside)")
    assert aside <= 0.25 * n_pairs
    assert ((g[:, None] - g[None, :])[told] > 0).all()


# ---------------------------------------------------------------------------------------------------- 5. batch independence
@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
def test_batch_equals_single_calls_bitwise(ctx, emb_mod, tok, precision):
    ids, eot = tok.encode_batch(R.TEXTS)
    m = _model(ctx, emb_mod, "small", precision)
    together = m.embed_ids_host(ids, eot)
    npads = []
    for i, text in enumerate(R.TEXTS):
        one_ids, one_eot = tok.encode_batch([text])
        npads.append(one_ids.shape[1])
        assert np.array_equal(m.embed_ids_host(one_ids, one_eot)[0], together[i]), f"text {i} depends on its batch"
    print(f"nine single calls of {npads} rows equal one call of {ids.shape[1]} rows, bitwise")
    assert npads == [8, 8, 8, 8, 8, 16, 24, 16, 80]
    assert np.abs(together[0] - together[1]).max() > 1e-3


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_embed_texts_is_independent_of_the_chunking(ctx, emb_mod, tok, precision):
    both = dict(V.make_state(V.SMALL, *V.GAINS["small"], seed=0), **_state("small"))
    e = emb_mod.ClipImageEmbeddings(state=both, precision=precision, ctx=ctx, tokenizer=tok)
    try:
        texts = [R.TEXTS[i] for i in (2, 8, 0, 5, 6)]
        whole = e.embed_texts(texts)
        assert (e.text_encoder_calls, e.texts_embedded) == (1, 5) and whole.shape == (5, 64)
        for chunk in (2, 1):
            assert np.array_equal(e.embed_texts(texts, chunk=chunk), whole)
        assert (e.text_encoder_calls, e.texts_embedded) == (1 + 3 + 5, 15)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 6. public surface
def test_public_surface(ctx, emb_mod, tok, vocab_dir):
    vision = V.make_state(V.SMALL, *V.GAINS["small"], seed=0)
    both = dict(vision, **_state("small"))
    torch.save({k: torch.from_numpy(v) for k, v in both.items()}, os.path.join(vocab_dir, "pytorch_model.bin"))
    with open(os.path.join(vocab_dir, "marie.json"), "w") as f:
        json.dump({"architecture": "ViT-B/32"}, f)
    e = emb_mod.OpenAIEmbeddings(vocab_dir, precision="f32", ctx=ctx)
    plain = emb_mod.ClipImageEmbeddings(state=vision, precision="f32", ctx=ctx)
    try:
        assert e.text_model is not None and e.context_length == 77
        out = e.get_embeddings(["the", "invoice"], image=None)
        ids, eot = tok.encode_batch(["the invoice"])
        _, want = R.forward(_state("small"), R.SMALL, ids, eot, torch.float32)
        err = np.abs(out.embeddings - want.numpy()).max()
        print(f"get_embeddings(['the', 'invoice']): max |d| {err:.3e}")
        assert out.embeddings.shape == (1, 64) and out.embeddings.dtype == np.float32 and out.total_tokens == -1
        assert err <= 1e-3
        assert np.array_equal(e.get_embeddings_raw(["the invoice"]), out.embeddings)
        with pytest.raises(ValueError, match="too long"):
            e.get_embeddings(["invoice"] * 76)
        assert e.get_embeddings(["invoice"] * 76, truncation=True).embeddings.shape == (1, 64)
        # pairs: duplicates are embedded once
        calls, count = e.text_encoder_calls, e.texts_embedded
        texts = ["the invoice total", "total", "the invoice total", "invoice total the", "total"]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 4), (3, 4)]
        cos, emb = e.text_cosine_pairs(texts, pairs, want_embeddings=True)
        ids, eot = tok.encode_batch(texts)
        _, ref = R.forward(_state("small"), R.SMALL, ids, eot, torch.float32)
        ref_cos = R.cosine_matrix(ref.double()).numpy()
        want_cos = np.array([ref_cos[a, b] for a, b in pairs])
        print(f"text_cosine_pairs: max |d cosine| {np.abs(cos - want_cos).max():.3e}; cosines {np.round(want_cos, 4)}")
        assert np.abs(cos - want_cos).max() <= 1e-5
        assert (e.text_encoder_calls, e.texts_embedded) == (calls + 1, count + 3)
        assert emb.shape == (5, 64) and np.array_equal(emb[0], emb[2]) and np.array_equal(emb[1], emb[4])
        assert np.array_equal(e.text_cosine_pairs(texts, pairs), cos)
        # the image side of the same instance is what it was
        clips = np.ascontiguousarray(V.make_clips()[[1, 5, 7]])
        assert np.array_equal(e.embed_clips(clips), plain.embed_clips(clips))
        assert (e.encoder_calls, e.clips_embedded) == (1, 3)
        # and without a text side the entry still refuses
        assert plain.text_model is None
        with pytest.raises(NotImplementedError, match="text"):
            plain.get_embeddings(["the", "invoice"])
        assert emb_mod.ClipImageEmbeddings(state=both, precision="f32", ctx=ctx, text=False).text_model is None
    finally:
        e.close()
        plain.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_create_and_calls_refuse_what_the_kernels_do_not_cover(ctx, emb_mod, tok):
    from marie_icr_amd._lib import ClipTextConfig, MarieHipError

    good = dict(vocab=R.VOCAB_SIZE, context=77, dim=128, heads=2, depth=2, ffn=512, proj_dim=64, ln_eps=1e-5)
    for change in (dict(dim=96), dict(heads=3), dict(dim=100, heads=1), dict(context=129), dict(ffn=100), dict(dim=2048, heads=32)):
        with pytest.raises(MarieHipError):
            emb_mod.ClipTextModel(ctx, None, ClipTextConfig(**dict(good, **change)), 1)
    m = _model(ctx, emb_mod, "small", 1)
    ids, eot = tok.encode_batch(["the invoice total", "total"])
    assert m.embed_ids_host(ids, eot).shape == (2, 64)

    def refused(i, e):
        with pytest.raises(MarieHipError):
            m.embed_ids_host(i, e)

    refused(np.zeros((2, 12), np.int32), eot)                    # rows no multiple of 8
    refused(np.zeros((2, 88), np.int32), eot)                    # more rows than the context rounded up to 8
    for bad in (-1, R.VOCAB_SIZE):
        changed = ids.copy()
        changed[1, 7] = bad
        refused(changed, eot)
    for bad in (0, 8, -1):
        refused(ids, np.array([bad, 2], np.int32))
    refused(np.zeros((4097, 8), np.int32), np.ones(4097, np.int32))
    with pytest.raises(MarieHipError):
        m.embed_pairs_host(ids, eot, [(0, 2)])
    unfinished = emb_mod.ClipTextModel(ctx, None, ClipTextConfig(**good), 1)
    with pytest.raises(MarieHipError):
        unfinished.embed_ids_host(ids, eot)
    unfinished.close()
