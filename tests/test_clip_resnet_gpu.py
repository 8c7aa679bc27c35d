"""CLIP's ModifiedResNet tower (csrc/cliprn_ops.hip, cliprn_api.hip), ``OpenAIResNetEmbeddings`` and the matcher's snippet score on
the GPU, against tests/clip_resnet_ref.py — the torch restatement tests/test_clip_resnet_cpu.py checks in float64 against numpy.

Bars:
  * the three kernels alone, against fp64: the project's 1e-3 absolute, on quantities each test asserts are O(1).  f16 mode
    works on f16-rounded inputs; its outputs are asserted to stay below 2, where the f16 rounding of an output is at most
    2^-11 * 2 = 4.9e-4 (the stem and the pool round their outputs; the attention pool rounds its tokens, a relative 2^-11 on
    every operand entry of the k | v product, and keeps everything after it in fp32);
  * fp32 mode against the fp32 restatement: taps and embeddings 1e-3, cosines 1e-5 (the ViT tests' bars);
  * f16 mode against the fp32 restatement: 2 x the constants below, measured on an MI355X; the order of two reference cosines
    is asserted only where their gap exceeds 4 x the cosine constant, and at most a quarter of the pairs may be set aside.
Every tower test asserts on the reference alone, over the eight clips of clip_ref.make_clips() brought to the model's size, that
one off-diagonal cosine lies below 0.7 and one above 0.99, that the largest embedding entry lies in [0.5, 10] and every tap's
largest entry in [0.5, 32].  Every test prints its figures before it asserts.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as V  # noqa: E402
import clip_resnet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# f16 model against the fp32 restatement, max over SMALL (B = 3), SMALL-96 (B = 3) and RN50x4 (B = 2) (first MI355X run: SMALL
# 1.611e-3 / 6.718e-4, SMALL-96 1.576e-3 / 7.087e-4, RN50x4 6.831e-3 / 3.314e-4; fp32 mode on the same cases: 4.2e-7 / 1.8e-7,
# 4.5e-7 / 1.3e-7 and 9.1e-6 / 7.8e-8)
F16_CLIPRN_EMBED_ERR_MEASURED = 6.831e-3    # max |d embedding entry| (entries up to 4.1)
F16_CLIPRN_COS_ERR_MEASURED = 7.087e-4      # max |d cosine| over all pairs of a case's clips

SMALL_288 = dict(R.SMALL, image_size=288)      # 82 tokens on the small width: the matcher's 224 x 224 clips go to 288
# config, gains, the clips of the case: noise, black and boxes (reference cosines 0.45 / 0.99 / 0.52 on SMALL: no two of them, nor
# one of them and the 1 of a clip with itself, closer than 0.01), black and boxes-with-a-bar (0.79) on RN50x4
CASES = {"small": (R.SMALL, "small", [0, 1, 5]), "small_96": (R.SMALL_96, "small_96", [0, 1, 5]),
         "rn50x4": (R.RN50X4, "rn50x4", [1, 7]), "small_288": (SMALL_288, "small", [1, 5, 7])}
_cache = {}


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


def _resized(clips_rgb, size):
    """uint8 RGB clips -> Pillow's BICUBIC (size, size) versions"""
    from PIL import Image

    return np.stack([np.asarray(Image.fromarray(c).resize((size, size), Image.BICUBIC)) for c in clips_rgb])


def _state(name):
    if ("state", name) not in _cache:
        cfg, gains, _ = CASES[name]
        _cache[("state", name)] = R.make_state(cfg, R.GAINS[gains], seed=0)
    return _cache[("state", name)]


def _check_reference(name, taps, emb):
    cos = V.cosine_matrix(emb.double()).numpy()
    off = cos[~np.eye(len(cos), dtype=bool)]
    tap_max = [float(t.abs().max()) for t in taps]
    print(f"{name}: reference cosines {off.min():.3f} .. {off.max():.4f}, largest embedding entry {float(emb.abs().max()):.2f}, "
          f"largest tap entries {['%.2f' % t for t in tap_max]}")
    assert off.min() < 0.7 and off.max() > 0.99, "the clips are not told apart"
    assert 0.5 <= float(emb.abs().max()) <= 10
    assert all(0.5 <= t <= 32 for t in tap_max)
    return cos


def _reference(name):
    """(clips of the case, their taps, embeddings, cosine matrix) from the fp32 restatement over all eight clips, computed once"""
    if ("ref", name) not in _cache:
        cfg, _, which = CASES[name]
        clips = _resized(V.make_clips(), cfg["image_size"])
        taps, emb = R.forward(_state(name), cfg, V.pixel_values(clips, torch.float32), torch.float32)
        cos = _check_reference(name, taps, emb)
        out = (np.ascontiguousarray(clips[which]), [t.numpy()[which] for t in taps], emb.numpy()[which], cos[np.ix_(which, which)])
        for a in (out[0], out[2], out[3], *out[1]):
            a.setflags(write=False)
        _cache[("ref", name)] = out
    return _cache[("ref", name)]


def _model(ctx, emb_mod, name, precision):
    tensors, cfg = emb_mod.load_clip_resnet_state(_state(name))
    return emb_mod.ClipResNetModel(ctx, tensors, cfg, precision)


def _all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- 1. the kernels alone
def _stem_case(S, C0, B, seed):
    rng = np.random.default_rng(seed)
    clips = rng.integers(0, 256, (B, S, S, 3)).astype(np.uint8)
    clips[0, 0, 0], clips[0, -1, -1] = 0, 255                  # the extremes, on the corners
    clips[..., 2] //= 2                                       # red and blue differ: a channel swap shows
    w = (0.05 * rng.standard_normal((C0, 3, 3, 3))).astype(np.float32)
    scale = (1 + 0.1 * rng.standard_normal(C0)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(C0)).astype(np.float32)
    return clips, w, scale, bias


def _stem_want(clips, w, scale, bias, swap_rb):
    rgb = clips[..., ::-1] if swap_rb else clips
    x = V.pixel_values(np.ascontiguousarray(rgb), torch.float64)
    y = torch.nn.functional.conv2d(x, torch.from_numpy(w).double(), stride=2, padding=1)      # zeros around the normalised clip
    y = torch.relu(y * torch.from_numpy(scale).double()[None, :, None, None] + torch.from_numpy(bias).double()[None, :, None, None])
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
@pytest.mark.parametrize("swap_rb", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C0", [8, 40])
@pytest.mark.parametrize("S", [8, 64])
def test_stem_kernel(ctx, emb_mod, S, C0, B, swap_rb, precision):
    clips, w, scale, bias = _stem_case(S, C0, B, S * 100 + C0 + B)
    got = emb_mod.resnet_stem_host(ctx, precision, clips, w, scale, bias, swap_rb=swap_rb)
    want = _stem_want(clips, w, scale, bias, swap_rb)
    other = _stem_want(clips, w, scale, bias, not swap_rb)
    err = float(np.abs(got - want).max())
    print(f"stem S={S} C0={C0} B={B} swap_rb={swap_rb} {'f32' if precision else 'f16'}: max |d| {err:.3e}, largest entry {want.max():.3f}, "
          f"zeros {float((want == 0).mean()):.2f}, channel order matters by {np.abs(want - other).max():.3f}")
    assert got.shape == want.shape == (B, S // 2, S // 2, C0)
    assert 0.5 <= want.max() <= 2 and 0.1 <= (want == 0).mean() <= 0.9          # O(1), and the ReLU cuts
    assert np.abs(want - other).max() > 0.05
    assert err <= 1e-3


@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (3, 6, 6, 40), (2, 18, 18, 320)])
def test_avgpool_kernel(ctx, emb_mod, shape, precision):
    rng = np.random.default_rng(sum(shape))
    x = (0.8 * rng.standard_normal(shape)).astype(np.float32)
    if precision == 0:
        x = _f16(x)                                           # what the kernel is handed
    got = emb_mod.avgpool_nhwc_host(ctx, precision, x)
    B, H, W, Cc = shape
    want = x.astype(np.float64).reshape(B, H // 2, 2, W // 2, 2, Cc).mean(axis=(2, 4))
    err = float(np.abs(got - want).max())
    print(f"avgpool {shape} {'f32' if precision else 'f16'}: max |d| {err:.3e}, largest entry {np.abs(want).max():.3f}")
    assert got.shape == want.shape and 0.5 <= np.abs(want).max() <= 2      # its f16 rounding is at most 2^-11 * 2 = 4.9e-4
    assert err <= 1e-3


def test_avgpool_refuses_what_it_does_not_cover(ctx, emb_mod):
    from marie_icr_amd._lib import MarieHipError

    for shape, k in (((1, 3, 2, 8), 2), ((1, 2, 5, 8), 2), ((1, 4, 4, 8), 4), ((1, 2, 2, 6), 2)):      # odd H, odd W, k = 4, C = 6
        for precision in (1, 0):
            with pytest.raises(MarieHipError):
                emb_mod.avgpool_nhwc_host(ctx, precision, np.ones(shape, np.float32), k=k)


def _attnpool_case(HW, E, P, B, sharp, seed):
    """the last map and the pool's weights; ``sharp``: the query projection times 6, so one key dominates most heads"""
    rng = np.random.default_rng(seed)
    n = lambda shape, s: (rng.standard_normal(shape) * s).astype(np.float32)
    x, pos = np.abs(n((B, HW, E), 1.0)), n((HW + 1, E), 0.5)            # the map comes out of a ReLU
    wq, wk, wv = (n((E, E), E ** -0.5) for _ in range(3))
    bq, bk, bv = (n((E,), 0.1) for _ in range(3))
    wc, bc = n((P, E), 0.5 * E ** -0.5), n((P,), 0.1)
    if sharp:
        wq, bq = wq * 6, bq * 6
    return x, pos, wq, bq, wk, bk, wv, bv, wc, bc


def _attnpool_want(x, pos, wq, bq, wk, bk, wv, bv, wc, bc):
    """fp64 -> (embeddings [B][P], the largest soft-max probability of every (clip, head))"""
    x, pos, wq, bq, wk, bk, wv, bv, wc, bc = (np.asarray(a, np.float64) for a in (x, pos, wq, bq, wk, bk, wv, bv, wc, bc))
    B, HW, E = x.shape
    tok = np.concatenate([x.mean(axis=1, keepdims=True), x], axis=1) + pos[None]
    q = ((tok[:, 0] @ wq.T + bq) * 64 ** -0.5).reshape(B, E // 64, 64)
    k = (tok @ wk.T + bk).reshape(B, HW + 1, E // 64, 64)
    v = (tok @ wv.T + bv).reshape(B, HW + 1, E // 64, 64)
    s = np.einsum("bhd,bthd->bht", q, k)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    ao = np.einsum("bht,bthd->bhd", p, v).reshape(B, E)
    return ao @ wc.T + bc, p.max(axis=-1)


ATTNPOOL_CASES = [(HW, E, P, B, False) for HW in (4, 9, 81) for E, P in ((512, 64), (2560, 640)) for B in (1, 3)] + \
                 [(81, 512, 64, 3, True), (9, 2560, 640, 1, True)]


@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
@pytest.mark.parametrize("HW,E,P,B,sharp", ATTNPOOL_CASES)
def test_attnpool_kernels(ctx, emb_mod, HW, E, P, B, sharp, precision):
    args = _attnpool_case(HW, E, P, B, sharp, HW * 7 + E + B)
    if precision == 0:                                        # what the f16 GEMMs are handed: the map and the three projections
        x, pos, wq, bq, wk, bk, wv, bv, wc, bc = args
        args = (_f16(x), pos, _f16(wq), bq, _f16(wk), bk, _f16(wv), bv, wc, bc)
    got = emb_mod.resnet_attnpool_host(ctx, precision, *args)
    want, pmax = _attnpool_want(*args)
    err = float(np.abs(got - want).max())
    print(f"attnpool {HW + 1} tokens E={E} P={P} B={B} sharp={sharp} {'f32' if precision else 'f16'}: max |d| {err:.3e}, largest entry "
          f"{np.abs(want).max():.3f}, largest probability of a head: mean {pmax.mean():.3f}, max {pmax.max():.3f}")
    assert got.shape == want.shape == (B, P) and 0.5 <= np.abs(want).max() <= 2
    if sharp:
        assert pmax.mean() > 0.6 and pmax.max() > 0.9         # one dominant key: the soft-max away from uniform
    else:
        assert pmax.mean() < 0.6
    assert err <= 1e-3


# ---------------------------------------------------------------------------------------------------- 2. fp32 mode
@pytest.mark.parametrize("name", ["small", "small_96", "rn50x4"])
def test_fp32_taps_embeddings_and_cosines(ctx, emb_mod, name):
    clips, ref_taps, ref_emb, ref_cos = _reference(name)
    m = _model(ctx, emb_mod, name, 1)
    try:
        taps, emb = m.debug_taps_host(clips)
        tap_err = [float(np.abs(t - r).max()) for t, r in zip(taps, ref_taps)]
        cos = m.embed_pairs_host(clips[..., ::-1], _all_pairs(len(clips))).reshape(len(clips), len(clips))
        print(f"{name} fp32: taps max |d| {['%.2e' % e for e in tap_err]}; embeddings {np.abs(emb - ref_emb).max():.3e}; "
              f"cosines {np.abs(cos - ref_cos).max():.3e}; workspace {m.workspace_bytes(len(clips))} bytes")
        assert [t.shape for t in taps] == [r.shape for r in ref_taps] and [m.tap_shape(i) for i in range(5)] == [r.shape[1:] for r in ref_taps]
        assert m.tap_shape(5) == (1, 1, m.cfg.proj_dim)
        for i, e in enumerate(tap_err):
            assert e <= 1e-3, f"tap {i} (0: the stem, k: layer k)"
        assert np.abs(emb - ref_emb).max() <= 1e-3
        assert np.abs(cos - ref_cos).max() <= 1e-5
        assert m.workspace_bytes(len(clips)) > clips.nbytes and m.workspace_bytes(0) == 0
    finally:
        m.close()


def test_padded_channels_leave_no_trace(ctx, emb_mod):
    """SMALL's channel counts are 8 (the stem's first two convolutions), 16 .. 512: in f16 mode every count below 64 is padded
    to 64, in fp32 mode 8 and 16 to 32.  The taps carry the reference's channel counts, and where the reference's ReLU gives
    exact zeros the tower does too"""
    clips, ref_taps, _, _ = _reference("small")
    assert [r.shape[-1] for r in ref_taps] == [16, 64, 128, 256, 512]
    for precision in (1, 0):
        m = _model(ctx, emb_mod, "small", precision)
        try:
            taps, _ = m.debug_taps_host(clips)
        finally:
            m.close()
        for i, (t, r) in enumerate(zip(taps, ref_taps)):
            assert t.shape == r.shape and np.isfinite(t).all()
            dead = (r == 0).all(axis=(0, 1, 2))               # channels the reference's ReLU silences everywhere
            assert not t[..., dead].any(), f"tap {i}"
            assert np.abs(t - r).max() <= (1e-3 if precision else 0.25), f"tap {i}"      # f16: placement only, the bars are above


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


@pytest.mark.parametrize("name", ["small", "small_96", "rn50x4"])
def test_f16_embeddings_and_cosines(ctx, emb_mod, name):
    emb, cos, e_emb, e_cos = _f16_errors(ctx, emb_mod, name)
    ref_cos = _reference(name)[3]
    print(f"{name} f16: max |d embedding| {e_emb:.3e}, max |d cosine| {e_cos:.3e} "
          f"(measured constants {F16_CLIPRN_EMBED_ERR_MEASURED}, {F16_CLIPRN_COS_ERR_MEASURED})")
    assert F16_CLIPRN_EMBED_ERR_MEASURED is not None, "the f16 embedding error has not been measured on an MI355X yet"
    assert F16_CLIPRN_COS_ERR_MEASURED is not None, "the f16 cosine error has not been measured on an MI355X yet"
    assert e_emb <= 2 * F16_CLIPRN_EMBED_ERR_MEASURED
    assert e_cos <= 2 * F16_CLIPRN_COS_ERR_MEASURED
    # the order of two cosines — those of the pairs of clips, and the 1 of a clip with itself — where the reference separates
    # them by more than both may move
    iu = np.triu_indices(len(cos), 1)
    r, g = np.concatenate([[1.0], ref_cos[iu]]), np.concatenate([[cos[0, 0]], cos[iu]])
    gap = r[:, None] - r[None, :]
    sure = gap > 4 * F16_CLIPRN_COS_ERR_MEASURED
    total = len(r) * (len(r) - 1) // 2
    aside = total - int(sure.sum())
    print(f"{name} f16: {int(sure.sum())} of {total} pairs of cosines checked for their order, {aside} set aside")
    assert cos[0, 0] == 1.0 and sure.any() and (g[:, None] > g[None, :])[sure].all()
    assert aside * 4 <= total


# ---------------------------------------------------------------------------------------------------- 4. batching
@pytest.mark.parametrize("precision", [1, 0], ids=["f32", "f16"])
def test_batch_equals_single_calls_bitwise(ctx, emb_mod, precision):
    clips = np.ascontiguousarray(_resized(V.make_clips()[[0, 1, 5, 7, 3]], 64))
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


def test_create_refuses_what_the_kernels_do_not_cover(ctx, emb_mod):
    import ctypes

    from marie_icr_amd._lib import ClipResNetConfig, MarieHipError

    C_INT4 = ctypes.c_int * 4

    def config(**kw):
        cfg = ClipResNetConfig(16, C_INT4(1, 2, 1, 1), 64, 64, 1e-5)
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    for kw, word in ((dict(image_size=80), "image_size"), (dict(image_size=544), "image_size"), (dict(width=15), "heads"),
                     (dict(width=130), "width"), (dict(layers=C_INT4(1, 0, 1, 1)), "layers")):
        with pytest.raises(MarieHipError, match=word):
            emb_mod.ClipResNetModel(ctx, None, config(**kw), 1)
    m = emb_mod.ClipResNetModel(ctx, None, config(), 1)
    with pytest.raises(MarieHipError):                        # no weights yet
        m.embed_host(np.zeros((1, 64, 64, 3), np.uint8))
    st = dict(_state("small"))
    del st["visual.layer3.0.bn2.running_var"]
    with pytest.raises(MarieHipError, match=r"visual\.layer3\.0\.bn2\.running_var"):      # finalize names what is missing
        m.load_state(st)
    m.close()


# ---------------------------------------------------------------------------------------------------- 5. the class
def test_get_embeddings_preprocesses_as_the_image_processor(ctx, emb_mod):
    from PIL import Image

    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, (260, 299, 3)).astype(np.uint8)
    src[60:200, 40:250] //= 3
    src[..., 2] //= 2                                         # red and blue differ: a channel swap shows
    image = Image.fromarray(src)
    e = emb_mod.OpenAIResNetEmbeddings(state={"model_state_dict": _state("small")}, precision="f32", ctx=ctx, text=None)
    try:
        assert e.image_size == 64 and e.proj_dim == 64 and e.text_model is None and e.architecture is None
        clip = e.preprocess(image)
        assert np.array_equal(clip, V.preprocess_u8(image, 64))           # the device resize is Pillow's, the crop the processor's
        out = e.get_embeddings([], image=image)
        _, want = R.forward(_state("small"), R.SMALL, V.pixel_values(clip[None], torch.float32), torch.float32)
        err = float(np.abs(out.embeddings - want.numpy()).max())
        print(f"get_embeddings on 299 x 260: max |d| {err:.3e}, largest entry {float(want.abs().max()):.2f}")
        assert out.embeddings.shape == (1, 64) and out.embeddings.dtype == np.float32 and out.total_tokens == -1
        # a noise image: a flatter embedding than the test clips' (the reference gives 0.49); 1e-3 is at most 0.4 % of 0.25
        assert 0.25 <= float(want.abs().max()) <= 10 and err <= 1e-3
        assert e.embed_clips(clip[None, ..., ::-1]).tobytes() == out.embeddings.tobytes()      # the matcher holds BGR clips
        assert np.abs(e.embed_clips(clip[None]) - out.embeddings).max() > 1e-3
        with pytest.raises(NotImplementedError):
            e.get_embeddings(["some", "text"])
    finally:
        e.close()


def test_embed_clips_brings_the_matchers_clips_to_the_models_size(ctx, emb_mod):
    """224 x 224 BGR clips on a 288 model: one Pillow-exact BICUBIC resize, then the tower"""
    clips, _, ref_emb, ref_cos = _reference("small_288")      # the restatement on Pillow's 288 x 288 versions
    small = np.ascontiguousarray(V.make_clips()[CASES["small_288"][2]][..., ::-1])      # 224 x 224, BGR
    e = emb_mod.OpenAIResNetEmbeddings(state=_state("small_288"), precision="f32", ctx=ctx, text=False)
    try:
        assert e.image_size == 288 and e.model.n_tok == 82
        calls = e.encoder_calls
        emb = e.embed_clips(small)
        cos, emb2 = e.cosine_pairs(small, _all_pairs(3), want_embeddings=True)
        print(f"embed_clips 224 -> 288: max |d| {np.abs(emb - ref_emb).max():.3e}, cosines {np.abs(cos.reshape(3, 3) - ref_cos).max():.3e}")
        assert e.encoder_calls == calls + 2 and e.clips_embedded >= 6
        assert np.abs(emb - ref_emb).max() <= 1e-3 and emb2.tobytes() == emb.tobytes()
        assert np.abs(cos.reshape(3, 3) - ref_cos).max() <= 1e-5
        assert e.embed_clips(np.ascontiguousarray(clips[..., ::-1])).tobytes() == emb.tobytes()      # already 288: taken as they are
    finally:
        e.close()


def test_matcher_scores_through_the_embeddings_object(ctx, emb_mod):
    from marie_icr_amd import template_matching as tmx
    from test_vqnnf_gpu import _page

    page, frames, boxes, labels, planted, stamps = _page()
    _reference("small")                                       # asserts that the weights tell the clips apart
    e = emb_mod.OpenAIResNetEmbeddings(state=_state("small"), precision="f32", ctx=ctx, architecture="RN-small")
    m = tmx.VQNNFTemplateMatcher("vqnnf", ctx=ctx, seed=5, embeddings_processor=e)
    try:
        bgr = [np.ascontiguousarray(c[..., ::-1]) for c in V.make_clips()]
        pairs = [(bgr[5], bgr[7]), (bgr[1], bgr[5]), (bgr[0], bgr[4]), (stamps["alpha"], stamps["beta"]), (stamps["alpha"], stamps["alpha"])]
        t_clips = np.stack([m._clip(t) for t, _ in pairs])
        q_clips = np.stack([m._clip(q) for _, q in pairs])
        both = _resized(np.concatenate([t_clips, q_clips])[..., ::-1], 64)           # what the reference's processor hands RN50x4
        _, ref = R.forward(_state("small"), R.SMALL, V.pixel_values(both, torch.float32), torch.float32)
        ref = ref.double()
        cos_ref = V.cosine(ref[:len(pairs)], ref[len(pairs):]).numpy()
        feature = tmx.clip_cosine_host(ctx, t_clips, q_clips).astype(np.float64)
        got = np.array(m.score_pairs(pairs, "weighted"))
        want = np.clip(0.05 * feature + 0.95 * cos_ref, 0, 1)
        print(f"matcher: reference cosines {cos_ref.tolist()}, features {feature.tolist()}, max |d score| {np.abs(got - want).max():.3e}")
        assert cos_ref.min() < 0.7 and cos_ref.max() > 0.99 and 0.5 <= float(ref.abs().max()) <= 10
        assert np.abs(got - want).max() <= 1e-5
        assert got[4] == 1.0 and m.score(stamps["beta"], stamps["beta"], "weighted") == 1.0      # identical snippets
        # one run over two pages: one encoder call per scoring batch (a page), every unique clip embedded once
        m.cached_embeddings_clips.clear()
        calls, embedded = e.encoder_calls, e.clips_embedded
        page2 = np.ascontiguousarray(page[:, ::-1])
        m.run([page, page2], frames, boxes, labels, window_size=(96, 128), max_objects=2, score_threshold=0.5)
        assert e.encoder_calls - calls == 2
        assert e.clips_embedded - embedded == len(m.cached_embeddings_clips)
    finally:
        m.close()
        e.close()


# ---------------------------------------------------------------------------------------------------- 6. the text side
def _text_embeddings(ctx, emb_mod, tmp_path_factory, text_cfg, precision="f32"):
    import cliptext_ref as T

    d = str(tmp_path_factory.mktemp("cliprn_text"))
    T.make_vocab(d)
    from marie_icr_amd.clip_tokenizer import ClipTokenizer

    tok = ClipTokenizer.from_dir(d)
    text_state = T.make_state(text_cfg, seed=0)
    both = dict(_state("small"), **text_state)
    e = emb_mod.OpenAIResNetEmbeddings(state=both, precision=precision, ctx=ctx, tokenizer=tok, text=True)
    return T, tok, text_state, e


def test_text_side_goes_through_the_existing_tower(ctx, emb_mod, tmp_path_factory):
    import cliptext_ref as T0

    T, tok, text_state, e = _text_embeddings(ctx, emb_mod, tmp_path_factory, T0.SMALL)
    try:
        assert e.text_model is not None and e.text_model.cfg.dim == 128 and e.context_length == 77
        texts = [T.TEXTS[i] for i in (2, 3, 5)]
        ids, eot = tok.encode_batch(texts)
        _, want = T.forward(text_state, T.SMALL, ids, eot, torch.float32)
        got = e.embed_texts(texts)
        one = e.get_embeddings(["the", "invoice", "total"]).embeddings
        print(f"text side, 128 wide: max |d| {np.abs(got - want.numpy()).max():.3e}, largest entry {float(want.abs().max()):.2f}")
        assert got.shape == (3, 64) and np.abs(got - want.numpy()).max() <= 1e-3
        assert one.tobytes() == got[:1].tobytes()             # get_embeddings joins its texts with a blank
    finally:
        e.close()


def test_text_tower_640_wide(ctx, emb_mod, tmp_path_factory):
    """RN50x4's text tower is 640 wide with 10 heads: the existing text tower takes it (a multiple of 64 up to 1024)"""
    import cliptext_ref as T0

    cfg = dict(T0.SMALL, dim=640, heads=10, ffn=2560, depth=2, proj_dim=640)
    T, tok, text_state, e = _text_embeddings(ctx, emb_mod, tmp_path_factory, cfg)
    try:
        assert e.text_model.cfg.dim == 640 and e.text_model.cfg.heads == 10
        ids, eot = tok.encode_batch(T.TEXTS)
        taps_ref, want = T.forward(text_state, cfg, ids, eot, torch.float32)
        taps, got = e.text_model.debug_taps_host(ids, eot)
        print(f"text tower 640 wide: taps max |d| {np.abs(taps - taps_ref.numpy()).max():.3e} (largest entry {float(taps_ref.abs().max()):.1f}), "
              f"embeddings {np.abs(got - want.numpy()).max():.3e} (largest entry {float(want.abs().max()):.2f})")
        assert got.shape == (len(T.TEXTS), 640) and 0.5 <= float(want.abs().max()) <= 10
        assert np.abs(got - want.numpy()).max() <= 1e-3
    finally:
        e.close()
