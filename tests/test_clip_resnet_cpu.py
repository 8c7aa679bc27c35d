"""CPU-side checks of the CLIP ModifiedResNet path: the torch restatement tests/clip_resnet_ref.py, the checkpoint loader and
the preprocessing arithmetic (no GPU).

The ``clip`` package is not installed, so there is no library to pin the restatement to.  Instead it is checked in float64
against code written independently of it in numpy: the attention pool from its formulas (mean token, positions, one query,
soft-max per head of 64, c_proj), and a Bottleneck of each kind and the stem's strided convolution from explicit loops over the
filter taps.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R  # noqa: E402
import clip_resnet_ref as RR  # noqa: E402


# ---------------------------------------------------------------------------------------------------- numpy, independently
def _np_conv(x, w, stride=1, pad=0):
    """x [n][C][H][W], w [O][C][k][k] -> [n][O][Ho][Wo], one filter tap at a time"""
    n, Cc, H, W = x.shape
    O, _, k, _ = w.shape
    xp = np.zeros((n, Cc, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = np.zeros((n, O, Ho, Wo))
    for dy in range(k):
        for dx in range(k):
            win = xp[:, :, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride]
            out += np.einsum("nchw,oc->nohw", win, w[:, :, dy, dx])
    return out


def _np_bn(x, st, p):
    g, b, mu, var = (np.asarray(st[p + "." + k], np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - mu[None, :, None, None]) / np.sqrt(var[None, :, None, None] + 1e-5) * g[None, :, None, None] + b[None, :, None, None]


def _np_pool(x):
    n, Cc, H, W = x.shape
    return x.reshape(n, Cc, H // 2, 2, W // 2, 2).mean(axis=(3, 5))


def _np_bottleneck(st, p, x, stride, down):
    w = lambda k: np.asarray(st[p + k + ".weight"], np.float64)
    out = np.maximum(_np_bn(_np_conv(x, w("conv1")), st, p + "bn1"), 0)
    out = np.maximum(_np_bn(_np_conv(out, w("conv2"), pad=1), st, p + "bn2"), 0)
    if stride > 1:
        out = _np_pool(out)
    out = _np_bn(_np_conv(out, w("conv3")), st, p + "bn3")
    idn = x
    if down:
        idn = _np_bn(_np_conv(_np_pool(x) if stride > 1 else x, w("downsample.0")), st, p + "downsample.1")
    return np.maximum(out + idn, 0)


def _np_attnpool(st, x, heads):
    """x [n][HW][E] -> [n][P]"""
    g = lambda k: np.asarray(st["visual.attnpool." + k], np.float64)
    n, HW, E = x.shape
    tok = np.concatenate([x.mean(axis=1, keepdims=True), x], axis=1) + g("positional_embedding")[None]
    q = (tok[:, 0] @ g("q_proj.weight").T + g("q_proj.bias")) * 64 ** -0.5
    k = tok @ g("k_proj.weight").T + g("k_proj.bias")
    v = tok @ g("v_proj.weight").T + g("v_proj.bias")
    out = np.zeros((n, E))
    for h in range(heads):
        sl = slice(h * 64, (h + 1) * 64)
        s = np.einsum("nd,ntd->nt", q[:, sl], k[:, :, sl])
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        out[:, sl] = np.einsum("nt,ntd->nd", p, v[:, :, sl])
    return out @ g("c_proj.weight").T + g("c_proj.bias")


@pytest.fixture(scope="module")
def small_state():
    return RR.make_state(RR.SMALL, RR.GAINS["small"], seed=0)


def test_restatement_agrees_with_numpy_blocks_and_attention_pool(small_state):
    st = small_state
    st64 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in st.items()}
    rng = np.random.default_rng(1)
    # the stem's strided convolution, zero padding around the normalised input
    x = rng.standard_normal((2, 3, 8, 8))
    want = _np_conv(x, np.asarray(st["visual.conv1.weight"], np.float64), stride=2, pad=1)
    got = torch.nn.functional.conv2d(torch.from_numpy(x), st64["visual.conv1.weight"], stride=2, padding=1).numpy()
    assert got.shape == (2, 8, 4, 4) and np.abs(got - want).max() <= 1e-12
    # a Bottleneck of each kind: downsample without a stride (layer1.0), with one (layer2.0), and none (layer2.1)
    kinds = {p: (cin, planes, stride, down) for p, cin, planes, stride, down in RR.blocks(RR.SMALL)}
    assert kinds["visual.layer1.0."][2:] == (1, True) and kinds["visual.layer2.0."][2:] == (2, True)
    assert kinds["visual.layer2.1."][2:] == (1, False)
    for p in ("visual.layer1.0.", "visual.layer2.0.", "visual.layer2.1."):
        cin, planes, stride, down = kinds[p]
        x = np.abs(rng.standard_normal((2, cin, 6, 6)))
        got = RR.bottleneck(st64, p, torch.from_numpy(x), stride, down).numpy()
        want = _np_bottleneck(st, p, x, stride, down)
        assert got.shape == (2, 4 * planes, 6 // stride, 6 // stride) and want.max() > 0.5
        assert np.abs(got - want).max() <= 1e-11, p
    # the attention pool, 5 and 10 tokens
    for cfg in (RR.SMALL, RR.SMALL_96):
        s = RR.make_state(cfg, RR.GAINS["small"], seed=3)
        s64 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in s.items()}
        g = cfg["image_size"] // 32
        x = rng.standard_normal((3, 512, g, g)) * 2
        got = RR.attnpool(s64, torch.from_numpy(x), 8).numpy()
        want = _np_attnpool(s, x.reshape(3, 512, g * g).transpose(0, 2, 1), 8)
        assert got.shape == (3, 64) and np.abs(want).max() > 0.5
        assert np.abs(got - want).max() <= 1e-11
    # and the whole tower: the taps are NHWC with the checkpoint's channel counts
    clips = R.make_clips(64)[[1, 5]]
    taps, emb = RR.forward(st, RR.SMALL, R.pixel_values(clips, torch.float64), torch.float64)
    assert [tuple(t.shape) for t in taps] == [(2, 16, 16, 16), (2, 16, 16, 64), (2, 8, 8, 128), (2, 4, 4, 256), (2, 2, 2, 512)]
    x = taps[4].permute(0, 3, 1, 2).numpy()
    assert np.abs(emb.numpy() - _np_attnpool(st, x.reshape(2, 512, 4).transpose(0, 2, 1), 8)).max() <= 1e-11


# ---------------------------------------------------------------------------------------------------- loader
@pytest.mark.parametrize("name,cfg", [("SMALL", RR.SMALL), ("RN50", RR.RN50), ("RN101", RR.RN101), ("RN50x4", RR.RN50X4)])
def test_loader_reads_the_geometry_from_the_shapes(name, cfg):
    from marie_icr_amd.embeddings import CLIP_RESNETS, clip_resnet_keys, load_clip_resnet_state

    sd = RR.make_state(cfg, (1.0, 0.0), zeros=True)
    tensors, c = load_clip_resnet_state(sd)
    assert (tuple(c.layers), c.width, c.image_size, c.proj_dim) == (tuple(cfg["layers"]), cfg["width"], cfg["image_size"], cfg["proj_dim"])
    assert c.embed_dim == 32 * cfg["width"] and c.heads == cfg["width"] // 2 and c.grid == cfg["image_size"] // 32
    assert abs(c.bn_eps - 1e-5) < 1e-12
    if name in CLIP_RESNETS:
        assert CLIP_RESNETS[name] == (tuple(cfg["layers"]), cfg["width"], cfg["image_size"], cfg["proj_dim"])
    assert set(tensors) == set(clip_resnet_keys(c)) == {k for k in sd if not k.endswith("num_batches_tracked")}
    assert all(v.dtype == np.float32 for v in tensors.values())


def test_rn50x4_geometry_is_the_published_one():
    from marie_icr_amd.embeddings import load_clip_resnet_state

    _, c = load_clip_resnet_state(RR.make_state(RR.RN50X4, (1.0, 0.0), zeros=True))
    assert (c.embed_dim, c.heads, c.grid ** 2 + 1) == (2560, 40, 82)


def test_loader_takes_both_wrappers_fp16_storage_and_extra_keys(small_state):
    from marie_icr_amd.embeddings import load_clip_resnet_state

    bare, _ = load_clip_resnet_state(small_state)
    half = {k: torch.from_numpy(np.asarray(v)).half() for k, v in small_state.items()}
    half["token_embedding.weight"] = torch.zeros(8, 4).half()          # the text tower and logit_scale are not the loader's
    half["logit_scale"] = torch.zeros(())
    wrapped, c = load_clip_resnet_state({"model_state_dict": half})
    assert set(wrapped) == set(bare) and c.width == 16
    assert not any(k.endswith("num_batches_tracked") for k in wrapped)
    for k in bare:
        assert wrapped[k].dtype == np.float32
        assert np.array_equal(wrapped[k], bare[k].astype(np.float16).astype(np.float32)), k


def test_loader_refusals(small_state):
    from marie_icr_amd._lib import MarieHipError
    from marie_icr_amd.embeddings import OpenAIResNetEmbeddings, load_clip_resnet_state

    vit = R.make_state(R.SMALL, 0.08, 0.01)
    with pytest.raises(MarieHipError, match="load_clip_vision_state"):
        load_clip_resnet_state(vit)
    with pytest.raises(MarieHipError, match="load_clip_vision_state"):
        load_clip_resnet_state({"model_state_dict": R.to_transformers(vit)})
    with pytest.raises(MarieHipError):
        load_clip_resnet_state({"model_state_dict": {"something.else": np.zeros(3, np.float32)}})
    sd = dict(small_state)
    del sd["visual.layer2.0.downsample.0.weight"]
    with pytest.raises(MarieHipError, match=r"visual\.layer2\.0\.downsample\.0\.weight"):
        load_clip_resnet_state(sd)
    sd = dict(small_state)
    sd["visual.attnpool.positional_embedding"] = np.zeros((7, 512), np.float32)      # 6 is no square
    with pytest.raises(MarieHipError, match="7 position rows"):
        load_clip_resnet_state(sd)
    sd = dict(small_state)
    sd["visual.layer3.0.conv2.weight"] = np.zeros((64, 64, 1, 1), np.float32)
    with pytest.raises(MarieHipError, match=r"visual\.layer3\.0\.conv2\.weight has shape"):
        load_clip_resnet_state(sd)
    # the class: an architecture that is no ModifiedResNet, or one that contradicts the shapes, before any device work
    with pytest.raises(ValueError, match="ViT-B/32"):
        OpenAIResNetEmbeddings(state=small_state, architecture="ViT-B/32")
    with pytest.raises(ValueError, match="RN50x4"):
        OpenAIResNetEmbeddings(state=small_state, architecture="RN50x4")


def test_marie_json_names_the_architecture(small_state, tmp_path):
    from marie_icr_amd.embeddings import OpenAIResNetEmbeddings

    model_dir = tmp_path / "clip-snippet-rn50x4"
    model_dir.mkdir()
    (model_dir / "marie.json").write_text(json.dumps({"_name_or_path": "marie/clip-snippet-rn50x4", "architecture": "RN50x4"}))
    with pytest.raises(ValueError, match="RN50x4"):              # read from marie.json, contradicted by the (small) shapes
        OpenAIResNetEmbeddings(str(model_dir), state=small_state)
    (model_dir / "marie.json").write_text(json.dumps({"architecture": "ViT-B/16"}))
    with pytest.raises(ValueError, match="ViT-B/16"):
        OpenAIResNetEmbeddings(str(model_dir), state=small_state)


def test_the_vit_classes_keep_refusing_and_name_the_new_class(small_state):
    from marie_icr_amd.embeddings import OpenAIEmbeddings, load_clip_vision_state

    with pytest.raises(NotImplementedError, match="OpenAIResNetEmbeddings"):
        OpenAIEmbeddings(architecture="RN50x4", state=small_state)
    with pytest.raises(NotImplementedError, match="load_clip_resnet_state"):
        load_clip_vision_state(small_state)


# ---------------------------------------------------------------------------------------------------- preprocessing
def test_preprocess_size_arithmetic_at_288():
    from marie_icr_amd.embeddings import center_crop_box, resized_size

    assert resized_size(224, 224, 288) == (288, 288) and center_crop_box(288, 288, 288) == (0, 0)      # the matcher's clip
    assert resized_size(299, 260, 288) == (331, 288) and center_crop_box(331, 288, 288) == (21, 0)     # int(288 * 299 / 260)
    assert resized_size(260, 299, 288) == (288, 331) and center_crop_box(288, 331, 288) == (0, 21)
    assert resized_size(1000, 289, 288) == (996, 288) and center_crop_box(996, 288, 288) == (354, 0)
    assert resized_size(288, 288, 288) == (288, 288)
    for w, h in ((299, 260), (260, 299), (224, 224), (1000, 289)):
        assert resized_size(w, h, 288) == R.resized_size(w, h, 288)


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_additions():
    import __graft_entry__ as g

    g.build()
    from marie_icr_amd import _lib

    lib = _lib.load()
    new = [s for s in _lib.EXPORTED_SYMBOLS if s.startswith("mhip_cliprn_")] + ["mhip_avgpool_nhwc_host"]
    assert sorted(new) == sorted(["mhip_cliprn_" + n for n in (
        "create", "destroy", "set_tensor", "finalize", "alloc_arena", "arena", "workspace_bytes", "embed_host", "embed_pairs_host",
        "tap_shape", "debug_taps_host", "stem_host", "attnpool_host")] + ["mhip_avgpool_nhwc_host"])
    for name in new:
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.ClipResNetConfig) == 8 * 4
