"""CPU-side checks of the CLIP image embeddings: tests/clip_ref.py (the restatement the GPU tests compare the HIP tower with)
against the transformers library in float64, its image processor against CLIPImageProcessor, the checkpoint loader of
marie_icr_amd/embeddings.py on both key schemes, the refusals, and the matcher's blend and cache with a counting fake."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R  # noqa: E402

transformers = pytest.importorskip("transformers")


@pytest.fixture(scope="module")
def small_state():
    return R.make_state(R.SMALL, *R.GAINS["small"], seed=0)


def test_restatement_equals_transformers_float64(small_state):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

    c = R.SMALL
    cfg = CLIPVisionConfig(hidden_size=c["dim"], intermediate_size=c["ffn"], num_hidden_layers=c["depth"],
                           num_attention_heads=c["heads"], image_size=c["image_size"], patch_size=c["patch"],
                           projection_dim=c["proj_dim"], hidden_act="quick_gelu", layer_norm_eps=1e-5)
    model = CLIPVisionModelWithProjection(cfg).double().eval()
    missing, unexpected = model.load_state_dict({k: v.double() for k, v in R.to_transformers(small_state).items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    pixels = R.pixel_values(R.make_clips(), torch.float64)
    with torch.no_grad():
        out = model(pixel_values=pixels, output_hidden_states=True)
    taps, emb = R.forward(small_state, c, pixels, torch.float64)
    err = float((out.image_embeds - emb).abs().max())
    print(f"max |restatement - transformers| embeddings {err:.3e}, largest entry {float(emb.abs().max()):.3f}")
    assert err <= 1e-12
    hs = out.hidden_states
    assert len(hs) == c["depth"] + 1
    for i, h in enumerate(hs):                     # after pre_layrnorm, then after every layer
        assert float((h - taps[i]).abs().max()) <= 1e-11, f"tap {i}"
    # the recipe tells the clips apart (the condition every GPU test carries)
    off = R.cosine_matrix(emb)[~torch.eye(len(emb), dtype=torch.bool)]
    assert off.min() < 0.7 and off.max() > 0.99 and 0.5 <= float(emb.abs().max()) <= 10


def _processor_pixels(image):
    from transformers import CLIPImageProcessor

    proc = CLIPImageProcessor()                    # openai/clip-vit-base-patch32's settings are the class defaults
    return np.asarray(proc(images=image, return_tensors="np")["pixel_values"])[0]


def _check_preprocessing(image):
    want = _processor_pixels(image)
    clip = R.preprocess_u8(image, 224)
    got = R.pixel_values(clip[None], torch.float32)[0].numpy()
    assert want.shape == got.shape == (3, 224, 224)
    # the uint8 clip behind the processor's floats, exactly; the floats to a few fp32 ulps of the normalised range
    back = np.rint((want.transpose(1, 2, 0).astype(np.float64) * np.array(R.CLIP_STD) + np.array(R.CLIP_MEAN)) * 255)
    assert np.array_equal(back.astype(np.uint8), clip)
    assert np.abs(want.astype(np.float64) - got).max() <= 2e-6
    return clip


def test_preprocessing_224_is_untouched():
    from PIL import Image

    src = np.random.default_rng(1).integers(0, 256, (224, 224, 3)).astype(np.uint8)
    assert np.array_equal(_check_preprocessing(Image.fromarray(src)), src)


def test_preprocessing_truncates_the_long_edge():
    """299 x 260 (w x h): the long edge scales to 257.6, int() gives 257 and round() 258 (300 x 260 gives 258 both ways)"""
    from PIL import Image
    from marie_icr_amd.embeddings import center_crop_box, resized_size

    assert int(224 * 299 / 260) == 257 and round(224 * 299 / 260) == 258
    assert R.resized_size(299, 260, 224) == (257, 224) == resized_size(299, 260, 224)
    assert resized_size(260, 299, 224) == (224, 257) and center_crop_box(257, 224, 224) == (16, 0)
    src = np.random.default_rng(2).integers(0, 256, (260, 299, 3)).astype(np.uint8)
    src[60:200, 40:250] //= 3                      # structure, so that a shift of one column shows
    _check_preprocessing(Image.fromarray(src))
    _check_preprocessing(Image.fromarray(np.ascontiguousarray(src.transpose(1, 0, 2))))      # portrait


def test_preprocessing_greyscale():
    from PIL import Image

    src = np.random.default_rng(3).integers(0, 256, (240, 230)).astype(np.uint8)
    clip = _check_preprocessing(Image.fromarray(src, mode="L"))
    assert np.array_equal(clip[..., 0], clip[..., 1]) and np.array_equal(clip[..., 1], clip[..., 2])


# ---------------------------------------------------------------------------------------------------- loader
def _openai_fp16(st):
    """the OpenAI-scheme checkpoint as clip saves it: torch tensors, fp16 storage, with some text-tower keys beside"""
    sd = {k: torch.from_numpy(v).half() for k, v in st.items()}
    sd["positional_embedding"] = torch.zeros(77, 64).half()
    sd["transformer.resblocks.0.attn.in_proj_weight"] = torch.zeros(192, 64).half()
    sd["logit_scale"] = torch.tensor(4.6)
    return sd


def test_loader_maps_both_key_schemes_to_the_same_tensors(small_state):
    from marie_icr_amd.embeddings import load_clip_vision_state

    # weights an fp16 checkpoint can hold exactly, so that both schemes carry the same numbers
    st = {k: v.astype(np.float16).astype(np.float32) for k, v in small_state.items()}
    hf = R.to_transformers(st)
    hf["text_model.embeddings.token_embedding.weight"] = torch.zeros(10, 64)
    hf["vision_model.embeddings.position_ids"] = torch.arange(50)[None]
    hf["logit_scale"] = torch.tensor(4.6)
    staged = [load_clip_vision_state(ck) for ck in (hf, {"model_state_dict": hf}, _openai_fp16(st),
                                                    {"model_state_dict": _openai_fp16(st)})]
    for tensors, cfg in staged:
        assert sorted(tensors) == sorted(st)
        for k, v in st.items():
            assert tensors[k].dtype == np.float32 and tensors[k].flags["C_CONTIGUOUS"]
            assert np.array_equal(tensors[k], v), k
        assert (cfg.dim, cfg.depth, cfg.heads, cfg.patch, cfg.image_size, cfg.ffn, cfg.proj_dim) == (128, 2, 2, 32, 224, 512, 64)
    t = staged[0][0]
    q = hf["vision_model.encoder.layers.1.self_attn.q_proj.weight"].numpy()
    v = hf["vision_model.encoder.layers.1.self_attn.v_proj.bias"].numpy()
    assert np.array_equal(t["visual.transformer.resblocks.1.attn.in_proj_weight"][:128], q)
    assert np.array_equal(t["visual.transformer.resblocks.1.attn.in_proj_bias"][256:], v)
    assert np.array_equal(t["visual.proj"], hf["visual_projection.weight"].numpy().T)


def test_loader_reads_the_geometry_from_the_shapes():
    from marie_icr_amd.embeddings import load_clip_vision_state

    b16 = dict(R.SMALL, patch=16)                  # 14 x 14 patches + class = 197 tokens
    _, cfg = load_clip_vision_state(R.make_state(b16, 0.05, 0.01, seed=1))
    assert (cfg.patch, cfg.image_size, cfg.dim, cfg.heads) == (16, 224, 128, 2)


def test_refusals(small_state, tmp_path):
    from marie_icr_amd._lib import MarieHipError
    from marie_icr_amd.embeddings import ClipImageEmbeddings, OpenAIEmbeddings, load_clip_vision_state

    with pytest.raises(NotImplementedError, match="RN50x4"):
        OpenAIEmbeddings(architecture="RN50x4", state=small_state)
    model_dir = tmp_path / "clip-snippet-rn50x4"
    model_dir.mkdir()
    (model_dir / "marie.json").write_text(json.dumps({"_name_or_path": "marie/clip-snippet-rn50x4", "architecture": "RN50x4"}))
    with pytest.raises(NotImplementedError, match="RN50x4"):
        OpenAIEmbeddings(str(model_dir))
    with pytest.raises(NotImplementedError, match="ResNet"):
        load_clip_vision_state({"visual.layer1.0.conv1.weight": np.zeros((4, 4, 1, 1), np.float32),
                                "visual.attnpool.positional_embedding": np.zeros((5, 4), np.float32)})
    with pytest.raises(MarieHipError):
        load_clip_vision_state({"model_state_dict": {"something.else": np.zeros(3, np.float32)}})
    # the text embedding is refused before any device work: no model is needed to see it
    bare = object.__new__(ClipImageEmbeddings)
    with pytest.raises(NotImplementedError, match="text"):
        bare.get_embeddings(["a", "b"], image=None)


# ---------------------------------------------------------------------------------------------------- matcher
class CountingEmbeddings:
    """the surface of embeddings.ClipImageEmbeddings the matcher uses, on the host, counting what it embeds"""

    def __init__(self):
        self.encoder_calls, self.embedded = 0, []

    def _one(self, clip):
        self.embedded.append(clip.tobytes())
        c = clip.astype(np.float64)
        return np.array([c[:112].mean(), c[112:].mean(), c[:, :112].mean(), c[:, 112:].mean(), 40.0], np.float32)

    def embed_clips(self, clips):
        self.encoder_calls += 1
        return np.stack([self._one(c) for c in clips])

    def pair_cosines(self, emb, pairs):
        emb = np.asarray(emb, np.float64)
        return np.array([emb[a] @ emb[b] / max(np.linalg.norm(emb[a]) * np.linalg.norm(emb[b]), 1e-8) for a, b in pairs], np.float32)

    def cosine_pairs(self, clips, pairs, want_embeddings=False):
        emb = self.embed_clips(clips)
        cos = self.pair_cosines(emb, pairs)
        return (cos, emb) if want_embeddings else cos


def _clip(seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (224, 224, 3)).astype(np.uint8)
    c[:112] //= (seed % 3 + 1)
    return c


@pytest.fixture()
def matcher(monkeypatch):
    from marie_icr_amd import template_matching as tmx

    fake = CountingEmbeddings()
    m = tmx.VQNNFTemplateMatcher("vqnnf", ctx=object(), embeddings_processor=fake)
    feature = {}
    monkeypatch.setattr(m, "_clip", lambda snippet: snippet)                    # the snippets below are clips already
    monkeypatch.setattr(tmx, "clip_cosine_host",
                        lambda ctx, a, b: np.array([feature.get((x.tobytes(), y.tobytes()), 0.5) for x, y in zip(a, b)], np.float32))
    return m, fake, feature


def test_matcher_blends_per_strategy_and_embeds_every_clip_once(matcher):
    m, fake, feature = matcher
    t0, t1, q = _clip(0), _clip(1), [_clip(10 + i) for i in range(3)]
    pairs = [(t0, q[0]), (t0, q[1]), (t1, q[1]), (t1, q[2]), (t0, t0)]
    for k, (a, b) in enumerate(pairs):
        feature[(a.tobytes(), b.tobytes())] = np.float32(0.3 + 0.1 * k)
    ref = CountingEmbeddings()
    want_e = [float(ref.pair_cosines(np.stack([ref._one(a), ref._one(b)]), [(0, 1)])[0]) for a, b in pairs]
    want_f = [float(np.float32(0.3 + 0.1 * k)) for k in range(len(pairs))]
    got = m.score_pairs(pairs, "weighted")
    assert got == pytest.approx([min(1, f * 0.05 + e * 0.95) for f, e in zip(want_f, want_e)], abs=1e-7)
    assert want_e[4] == pytest.approx(1.0, abs=1e-7)
    assert fake.encoder_calls == 1 and len(fake.embedded) == 5 == len(set(fake.embedded))      # t0, t1, q0, q1, q2: once each
    assert m.score_pairs(pairs, "max") == pytest.approx([min(1, max(f, e)) for f, e in zip(want_f, want_e)], abs=1e-7)
    assert m.score_pairs(pairs, "average") == pytest.approx([(f + e) / 2 for f, e in zip(want_f, want_e)], abs=1e-7)
    assert fake.encoder_calls == 1                                             # everything was cached: no further embed
    # the next page: the templates are known, two new query clips take one encoder call
    q2 = [_clip(20), _clip(21)]
    for a, b in ((t0, q2[0]), (t1, q2[1])):
        feature[(a.tobytes(), b.tobytes())] = np.float32(0.5)
    m.score_pairs([(t0, q2[0]), (t1, q2[1])], "weighted")
    assert fake.encoder_calls == 2 and len(fake.embedded) == 7 == len(set(fake.embedded))
    # single clips are served from the same cache, and a new one is embedded once
    before = len(fake.embedded)
    assert np.array_equal(m.get_embedding_feature(t0), ref._one(t0))
    extra = _clip(30)
    m.get_embedding_feature(extra)
    m.get_embedding_feature(extra)
    assert len(fake.embedded) == before + 1
    with pytest.raises(ValueError):
        m.score_pairs([(t0, np.zeros((100, 224, 3), np.uint8))], "weighted")


def test_matcher_without_an_object_scores_as_before(monkeypatch):
    from marie_icr_amd import template_matching as tmx

    a, b = _clip(1), _clip(2)
    monkeypatch.setattr(tmx, "clip_cosine_host", lambda ctx, x, y: np.array([0.25] * len(x), np.float32))
    for proc, emb_sim in ((None, 0.25), (lambda clip: clip.reshape(-1)[:4].astype(np.float64) + 1, None)):
        m = tmx.VQNNFTemplateMatcher("vqnnf", ctx=object(), embeddings_processor=proc)
        monkeypatch.setattr(m, "_clip", lambda snippet: snippet)
        if emb_sim is None:
            x, y = proc(a), proc(b)
            emb_sim = float(x @ y / (np.linalg.norm(x) * np.linalg.norm(y)))
        assert m.score(a, b, "weighted") == pytest.approx(0.25 * 0.05 + emb_sim * 0.95, abs=1e-12)
    comp = tmx.CompositeTemplateMatcher([m, tmx.VQNNFTemplateMatcher("vqnnf", ctx=object())], embeddings_processor="object")
    assert comp.matchers[0].embeddings_processor is proc and comp.matchers[1].embeddings_processor == "object"
