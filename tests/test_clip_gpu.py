"""The CLIP vision tower (csrc/clip_ops.hip, clip_api.hip), the embeddings classes and the matcher's snippet score on the GPU,
against tests/clip_ref.py — the torch restatement tests/test_clip_cpu.py pins to the transformers library in float64.

Bars:
  * the four row kernels alone, against fp64: the project's 1e-3 absolute, on quantities each test asserts are O(1);
  * fp32 mode against the fp32 restatement: residual-stream taps and embeddings 1e-3, cosines 1e-5 (the bars the classifier and
    the splitter carry for logits and scores);
  * f16 mode against the fp32 restatement: 2 x the constants below, measured on an MI355X; the order of two reference cosines
    is asserted only where their gap exceeds 2 x the cosine bound.
Every GPU test on the tower asserts that its reference cosines include one below 0.7 and one above 0.99 and that the largest
reference embedding entry lies in [0.5, 10]: the absolute bars mean something only on embeddings that tell the clips apart.
Every test prints its figures before it asserts.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# f16 model against the fp32 restatement, max over the small config at B = 3 and ViT-B/32 at B = 8 (first MI355X run:
# small 1.304e-3 / 5.70e-5, ViT-B/32 2.301e-3 / 1.663e-4)
F16_CLIP_EMBED_ERR_MEASURED = 2.301e-3   # max |d embedding entry| (entries up to 2.7)
F16_CLIP_COS_ERR_MEASURED = 1.663e-4     # max |d cosine| over all pairs of a case's clips

CLIPS = R.make_clips()
CASES = {"small": (R.SMALL, [1, 5, 7]), "vit_b32": (R.VIT_B32, list(range(8)))}      # config, the clips of the case
_ref_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emb_mod():
    from marie_icr_amd import embeddings

    return embeddings


def _state(name):
    if ("state", name) not in _ref_cache:
        _ref_cache[("state", name)] = R.make_state(CASES[name][0], *R.GAINS[name], seed=0)
    return _ref_cache[("state", name)]


def _reference(name):
    """(clips, taps, embeddings, cosine matrix) of a case from the fp32 restatement, computed once"""
    if name not in _ref_cache:
        cfg, which = CASES[name]
        clips = np.ascontiguousarray(CLIPS[which])
        taps, emb = R.forward(_state(name), cfg, R.pixel_values(clips, torch.float32), torch.float32)
        taps, emb = taps.numpy(), emb.numpy()
        cos = R.cosine_matrix(torch.from_numpy(emb).double()).numpy()
        off = cos[~np.eye(len(cos), dtype=bool)]
        assert off.min() < 0.7 and off.max() > 0.99, "the clips are not told apart"
        assert 0.5 <= np.abs(emb).max() <= 10
        for a in (clips, taps, emb, cos):
            a.setflags(write=False)
        _ref_cache[name] = (clips, taps, emb, cos)
    return _ref_cache[name]


def _model(ctx, emb_mod, name, precision):
    tensors, cfg = emb_mod.load_clip_vision_state(_state(name))
    return emb_mod.ClipVisionModel(ctx, tensors, cfg, precision)


def _all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


# ---------------------------------------------------------------------------------------------------- 1. the kernels alone
@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
def test_quick_gelu_kernel(ctx, emb_mod, precision):
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-3.5, 3.5, 4093), [20.0, -20.0, 0.0]]).astype(np.float32)     # 4096 values, two blocks
    if precision == 0:
        x = x.astype(np.float16).astype(np.float32)          # what the kernel is handed
    got = emb_mod.quick_gelu_host(ctx, precision, x)
    x64 = x.astype(np.float64)
    want = x64 / (1.0 + np.exp(-1.702 * x64))
    err = np.abs(got - want)
    print(f"quick_gelu {'f32' if precision else 'f16'}: max |d| {err[:-3].max():.3e} on |x| <= 3.5, at +20 / -20 / 0: {got[-3:].tolist()}")
    assert np.abs(want[:-3]).max() <= 4.0                     # O(1): below 4 an f16 output carries at most 2^-10 = 9.8e-4 of rounding
    assert err[:-3].max() <= 1e-3
    assert got[-3] == 20.0 and abs(got[-2]) <= 1e-12 and got[-1] == 0.0


@pytest.mark.parametrize("B,D", [(1, 128), (3, 128), (3, 768)])
def test_embed_kernel(ctx, emb_mod, B, D):
    rng = np.random.default_rng(B * 1000 + D)
    n_tok = 50
    patches = rng.standard_normal((B, n_tok - 1, D)).astype(np.float32)
    cls, pos = rng.standard_normal(D).astype(np.float32), (0.5 * rng.standard_normal((n_tok, D))).astype(np.float32)
    g, b = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)
    got = emb_mod.embed_rows_host(ctx, patches, cls, pos, g, b, 1e-5)
    x = np.concatenate([np.broadcast_to(cls, (B, 1, D)), patches], axis=1).astype(np.float64) + pos
    want = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5) * g + b
    err = float(np.abs(got[:, :n_tok] - want).max())
    print(f"embed B={B} D={D}: max |d| {err:.3e}, largest entry {np.abs(want).max():.3f}")
    assert got.shape == (B, 56, D) and 0.5 <= np.abs(want).max() <= 10
    assert err <= 1e-3
    assert not got[:, n_tok:].any()                           # the padding rows are zeros


@pytest.mark.parametrize("B,D,E", [(1, 128, 64), (3, 128, 64), (3, 768, 512)])
def test_head_kernel(ctx, emb_mod, B, D, E):
    rng = np.random.default_rng(B * 1000 + D)
    h = (3 * rng.standard_normal((B, 56, D))).astype(np.float32)
    g, b = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)
    proj = (rng.standard_normal((D, E)) / np.sqrt(D)).astype(np.float32)
    got = emb_mod.head_host(ctx, h, g, b, proj, 1e-5)
    x = h[:, 0].astype(np.float64)
    want = ((x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5) * g + b) @ proj.astype(np.float64)
    err = float(np.abs(got - want).max())
    print(f"head B={B} D={D} E={E}: max |d| {err:.3e}, largest entry {np.abs(want).max():.3f}")
    assert 0.5 <= np.abs(want).max() <= 10
    assert err <= 1e-3


def test_pair_cosine_kernel(ctx, emb_mod):
    rng = np.random.default_rng(4)
    emb = rng.standard_normal((6, 512)).astype(np.float32)
    emb[2] = emb[1] + 0.05 * rng.standard_normal(512)        # a near pair
    emb[4] = 0                                               # a zero vector
    emb[5] = emb[0, :512] * 3                                # a scaled copy: cosine 1 up to rounding
    pairs = _all_pairs(6) + [(3, 3)]
    got = emb_mod.pair_cosine_host(ctx, emb, pairs)
    e = emb.astype(np.float64)
    want = np.array([e[a] @ e[b] / max(np.linalg.norm(e[a]) * np.linalg.norm(e[b]), 1e-8) for a, b in pairs])
    err = float(np.abs(got - want).max())
    print(f"pair cosine: max |d| {err:.3e}; self pairs {[float(got[i * 6 + i]) for i in range(6)]}")
    assert err <= 1e-5 and np.abs(want).max() <= 1.0 + 1e-12
    for i in (0, 1, 2, 3, 5):
        assert got[i * 6 + i] == 1.0                          # a vector with itself: exactly 1
    assert got[4 * 6 + 4] == 0.0 and not got[4 * 6: 5 * 6].any()      # the zero vector: 0 / max(0, 1e-8)
    narrow = emb_mod.pair_cosine_host(ctx, emb[:, :40], [(1, 2), (0, 5)])           # a width below one wave
    want_12 = (e[1, :40] @ e[2, :40]) / (np.linalg.norm(e[1, :40]) * np.linalg.norm(e[2, :40]))
    assert abs(narrow[0] - want_12) <= 1e-5 and abs(narrow[1] - 1.0) <= 1e-6


# ---------------------------------------------------------------------------------------------------- 2. fp32 mode
@pytest.mark.parametrize("name", ["small", "vit_b32"])
def test_fp32_taps_embeddings_and_cosines(ctx, emb_mod, name):
    clips, ref_taps, ref_emb, ref_cos = _reference(name)
    m = _model(ctx, emb_mod, name, 1)
    try:
        taps, emb = m.debug_taps_host(clips)
        tap_err = [float(np.abs(taps[i] - ref_taps[i]).max()) for i in range(len(taps))]
        cos = m.embed_pairs_host(clips[..., ::-1], _all_pairs(len(clips))).reshape(len(clips), len(clips))
        print(f"{name} fp32: taps max |d| {['%.2e' % e for e in tap_err]} (largest entry {np.abs(ref_taps).max():.2f}); "
              f"embeddings {np.abs(emb - ref_emb).max():.3e}; cosines {np.abs(cos - ref_cos).max():.3e}; "
              f"workspace {m.workspace_bytes(len(clips))} bytes")
        assert taps.shape == ref_taps.shape
        for i, e in enumerate(tap_err):
            assert e <= 1e-3, f"tap {i} (0: the embedding kernel, k: layer k)"
        assert np.abs(emb - ref_emb).max() <= 1e-3
        assert np.abs(cos - ref_cos).max() <= 1e-5
        assert m.workspace_bytes(len(clips)) > clips.nbytes and m.workspace_bytes(0) == 0
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------- 3. f16 mode
def _f16_errors(ctx, emb_mod, name):
    clips, _, ref_emb, ref_cos = _reference(name)
    m = _model(ctx, emb_mod, name, 0)
    try:
        n = len(clips)
        cos, emb = m.embed_pairs_host(clips[..., ::-1], _all_pairs(n), want_embeddings=True)
    finally:
        m.close()
    return emb, cos.reshape(n, n), float(np.abs(emb - ref_emb).max()), float(np.abs(cos.reshape(n, n) - ref_cos).max())


@pytest.mark.parametrize("name", ["small", "vit_b32"])
def test_f16_embeddings_and_cosines(ctx, emb_mod, name):
    emb, cos, e_emb, e_cos = _f16_errors(ctx, emb_mod, name)
    ref_cos = _reference(name)[3]
    print(f"{name} f16: max |d embedding| {e_emb:.3e}, max |d cosine| {e_cos:.3e} "
          f"(measured constants {F16_CLIP_EMBED_ERR_MEASURED}, {F16_CLIP_COS_ERR_MEASURED})")
    assert F16_CLIP_EMBED_ERR_MEASURED is not None, "the f16 embedding error has not been measured on an MI355X yet"
    assert F16_CLIP_COS_ERR_MEASURED is not None, "the f16 cosine error has not been measured on an MI355X yet"
    emb_bound, cos_bound = 2 * F16_CLIP_EMBED_ERR_MEASURED, 2 * F16_CLIP_COS_ERR_MEASURED
    assert e_emb <= emb_bound
    assert e_cos <= cos_bound
    # the order of two cosines, where the reference separates them by more than both may move
    iu = np.triu_indices(len(cos), 1)
    r, g = ref_cos[iu], cos[iu]
    gap = r[:, None] - r[None, :]
    sure = gap > 2 * cos_bound
    print(f"{name} f16: {int(sure.sum())} of {gap.size} ordered pairs of cosines checked")
    assert sure.any() and (g[:, None] > g[None, :])[sure].all()


# ---------------------------------------------------------------------------------------------------- 4. batching
@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
def test_batch_equals_single_calls_bitwise(ctx, emb_mod, precision):
    clips = np.ascontiguousarray(CLIPS[[0, 1, 5, 7, 3]])
    m = _model(ctx, emb_mod, "small", precision)
    try:
        together = m.embed_host(clips)
        singles = np.concatenate([m.embed_host(clips[i:i + 1]) for i in range(5)])
        assert together.tobytes() == singles.tobytes()
        pairs = _all_pairs(5)
        cos, emb = m.embed_pairs_host(clips, pairs, want_embeddings=True)
        bgr = m.embed_host(clips, swap_rb=True)               # the pairs entry takes BGR clips
        assert emb.tobytes() == bgr.tobytes()
        assert cos.tobytes() == emb_mod.pair_cosine_host(ctx, bgr, pairs).tobytes()
        assert np.abs(bgr - together).max() > 1e-3            # and the channel order matters
    finally:
        m.close()


def test_vit_b16_geometry_runs_through_the_same_code(ctx, emb_mod):
    """197 tokens (14 x 14 patches of 16 + class): four 64-key tiles, two 128-query blocks, 200 rows a clip"""
    cfg = dict(R.SMALL, patch=16)
    st = R.make_state(cfg, 0.08, 0.01, seed=2)
    clips = np.ascontiguousarray(CLIPS[[1, 5, 7]])
    taps_ref, emb_ref = R.forward(st, cfg, R.pixel_values(clips, torch.float32), torch.float32)
    tensors, c = emb_mod.load_clip_vision_state(st)
    m = emb_mod.ClipVisionModel(ctx, tensors, c, 1)
    try:
        taps, emb = m.debug_taps_host(clips)
    finally:
        m.close()
    print(f"ViT-*/16 small: taps {np.abs(taps - taps_ref.numpy()).max():.3e}, embeddings {np.abs(emb - emb_ref.numpy()).max():.3e}")
    assert taps.shape == (3, 3, 197, 128) and 0.5 <= np.abs(emb_ref.numpy()).max() <= 10
    assert np.abs(taps - taps_ref.numpy()).max() <= 1e-3 and np.abs(emb - emb_ref.numpy()).max() <= 1e-3


def test_create_refuses_what_the_kernels_do_not_cover(ctx, emb_mod):
    from marie_icr_amd._lib import ClipVisConfig, MarieHipError

    for field, value in (("heads", 4), ("patch", 14), ("ffn", 500), ("dim", 2048)):      # head dim 32; 3 * 14 * 14 columns; ...
        cfg = ClipVisConfig(128, 2, 2, 32, 224, 512, 64, 1e-5)
        setattr(cfg, field, value)
        if field == "dim":
            cfg.heads = 32
        with pytest.raises(MarieHipError):
            emb_mod.ClipVisionModel(ctx, None, cfg, 1)
    m = emb_mod.ClipVisionModel(ctx, None, ClipVisConfig(128, 2, 2, 32, 224, 512, 64, 1e-5), 1)
    with pytest.raises(MarieHipError):                        # no weights yet
        m.embed_host(CLIPS[:1])
    m.close()


# ---------------------------------------------------------------------------------------------------- 5. host path
def test_get_embeddings_preprocesses_as_the_image_processor(ctx, emb_mod):
    from PIL import Image

    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, (260, 299, 3)).astype(np.uint8)
    src[60:200, 40:250] //= 3
    src[..., 2] //= 2                                         # red and blue differ: a channel swap shows
    image = Image.fromarray(src)
    e = emb_mod.OpenAITransformerEmbeddings(state={"model_state_dict": R.to_transformers(_state("small"))}, precision="f32", ctx=ctx)
    try:
        clip = e.preprocess(image)
        assert np.array_equal(clip, R.preprocess_u8(image, 224))           # the device resize is Pillow's, the crop the processor's
        out = e.get_embeddings([], image=image)
        _, want = R.forward(_state("small"), R.SMALL, R.pixel_values(clip[None], torch.float32), torch.float32)
        err = float(np.abs(out.embeddings - want.numpy()).max())
        print(f"get_embeddings on 299 x 260: max |d| {err:.3e}")
        assert out.embeddings.shape == (1, 64) and out.embeddings.dtype == np.float32 and out.total_tokens == -1
        assert err <= 1e-3
        # the matcher holds BGR clips: the same pixels stored BGR give the same embedding, stored RGB a different one
        assert e.embed_clips(clip[None, ..., ::-1]).tobytes() == out.embeddings.tobytes()
        assert np.abs(e.embed_clips(clip[None]) - out.embeddings).max() > 1e-3
        grey = e.get_embeddings([], image=Image.fromarray(src[..., 0], mode="L")).embeddings
        _, want = R.forward(_state("small"), R.SMALL, R.pixel_values(R.preprocess_u8(Image.fromarray(src[..., 0], mode="L"))[None]), torch.float32)
        assert np.abs(grey - want.numpy()).max() <= 1e-3
        with pytest.raises(NotImplementedError):
            e.get_embeddings(["some", "text"])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- 6. matcher end to end
def test_matcher_scores_through_the_embeddings_object(ctx, emb_mod):
    from marie_icr_amd import template_matching as tmx
    from test_vqnnf_gpu import _page

    page, frames, boxes, labels, planted, stamps = _page()
    e = emb_mod.OpenAIEmbeddings(state=_state("small"), precision="f32", ctx=ctx, architecture="ViT-B/32")
    m = tmx.VQNNFTemplateMatcher("vqnnf", ctx=ctx, seed=5, embeddings_processor=e)
    try:
        # score == 0.05 * feature + 0.95 * reference cosine, on snippet pairs the reference tells apart
        bgr = [np.ascontiguousarray(c[..., ::-1]) for c in CLIPS]
        pairs = [(bgr[5], bgr[7]), (bgr[1], bgr[5]), (bgr[0], bgr[4]), (stamps["alpha"], stamps["beta"]), (stamps["alpha"], stamps["alpha"])]
        t_clips = np.stack([m._clip(t) for t, _ in pairs])
        q_clips = np.stack([m._clip(q) for _, q in pairs])
        both = np.concatenate([t_clips, q_clips])[..., ::-1]
        _, ref = R.forward(_state("small"), R.SMALL, R.pixel_values(np.ascontiguousarray(both), torch.float32), torch.float32)
        ref = ref.double()
        cos_ref = R.cosine(ref[:len(pairs)], ref[len(pairs):]).numpy()
        feature = tmx.clip_cosine_host(ctx, t_clips, q_clips).astype(np.float64)
        got = np.array(m.score_pairs(pairs, "weighted"))
        want = np.clip(0.05 * feature + 0.95 * cos_ref, 0, 1)
        print(f"matcher: reference cosines {cos_ref.tolist()}, features {feature.tolist()}, max |d score| {np.abs(got - want).max():.3e}")
        assert cos_ref.min() < 0.7 and cos_ref.max() > 0.99 and 0.5 <= float(ref.abs().max()) <= 10
        assert np.abs(got - want).max() <= 1e-5
        assert got[4] == 1.0 and m.score(stamps["beta"], stamps["beta"], "weighted") == 1.0      # identical snippets
        assert np.array(m.score_pairs(pairs, "max")) == pytest.approx(np.clip(np.maximum(feature, cos_ref), 0, 1), abs=1e-5)
        # one run over two pages: one encoder call per scoring batch (a page), every unique clip embedded once
        m.cached_embeddings_clips.clear()
        calls, embedded = e.encoder_calls, e.clips_embedded
        page2 = np.ascontiguousarray(page[:, ::-1])
        m.run([page, page2], frames, boxes, labels, window_size=(96, 128), max_objects=2, score_threshold=0.5)
        assert e.encoder_calls - calls == 2
        assert e.clips_embedded - embedded == len(m.cached_embeddings_clips)
        template_keys = {m._clip(f[b[1]:b[1] + b[3], b[0]:b[0] + b[2]]).tobytes() for f, b in zip(frames, boxes)}
        assert template_keys <= set(m.cached_embeddings_clips)
        # a second run: the known pages cost no encoder call, a new page embeds its query clips only
        calls, embedded, known = e.encoder_calls, e.clips_embedded, set(m.cached_embeddings_clips)
        m.run([page], frames, boxes, labels, window_size=(96, 128), max_objects=2, score_threshold=0.5)
        assert e.encoder_calls == calls
        m.run([np.ascontiguousarray(page[::-1])], frames, boxes, labels, window_size=(96, 128), max_objects=2, score_threshold=0.5)
        new = set(m.cached_embeddings_clips) - known
        print(f"matcher: {len(known)} clips after two pages, {len(new)} new on the third")
        assert e.encoder_calls == calls + 1 and e.clips_embedded - embedded == len(new) and new and not (new & template_keys)
        assert m.template_builds == 2
    finally:
        m.close()
        e.close()
