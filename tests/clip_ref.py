"""Plain-torch restatement of the CLIP vision tower + projection and of its image processor, parameterised by dtype (test
infrastructure: the GPU tests compare the HIP model against it, the CPU tests compare it against the transformers library in
float64), plus the seeded weights and the eight test clips both use.

Follows transformers/models/clip/modeling_clip.py: CLIPVisionEmbeddings, CLIPVisionTransformer (pre_layrnorm, CLIPEncoderLayer
with quick_gelu, post_layernorm on the class row), CLIPVisionModelWithProjection.visual_projection; and
image_processing_clip.py: convert RGB, BICUBIC shortest-edge resize, centre crop, rescale 1 / 255, normalise.  Weights are
taken under the OpenAI key scheme (``visual.*``), which is what marie_icr_amd.embeddings.load_clip_vision_state stages.
"""
from __future__ import annotations

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

SMALL = dict(dim=128, depth=2, heads=2, ffn=512, proj_dim=64, patch=32, image_size=224)
VIT_B32 = dict(dim=768, depth=12, heads=12, ffn=3072, proj_dim=512, patch=32, image_size=224)
# the gains of the seeded recipe (the issue's table): every other >= 2-d weight N(0, g_w), class / position N(0, g_cls)
GAINS = {"small": (0.08, 0.01), "vit_b32": (0.03, 0.02)}


def make_state(cfg: dict, g_w: float, g_cls: float, seed: int = 0) -> dict:
    """seeded OpenAI-scheme weights (float32 arrays): patch embedding N(0, 0.02), class / position embeddings N(0, g_cls),
    every other >= 2-d weight N(0, g_w), biases N(0, 0.1), LayerNorm gains 1 + 0.1 N"""
    rng = np.random.default_rng(seed)
    D, F, E, P = cfg["dim"], cfg["ffn"], cfg["proj_dim"], cfg["patch"]
    n_tok = (cfg["image_size"] // P) ** 2 + 1

    def n(shape, s):
        return (rng.standard_normal(shape) * s).astype(np.float32)

    def ln(prefix, st):
        st[prefix + ".weight"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        st[prefix + ".bias"] = n((D,), 0.1)

    st = {"visual.conv1.weight": n((D, 3, P, P), 0.02), "visual.class_embedding": n((D,), g_cls),
          "visual.positional_embedding": n((n_tok, D), g_cls)}
    ln("visual.ln_pre", st)
    for i in range(cfg["depth"]):
        p = f"visual.transformer.resblocks.{i}."
        ln(p + "ln_1", st)
        st[p + "attn.in_proj_weight"], st[p + "attn.in_proj_bias"] = n((3 * D, D), g_w), n((3 * D,), 0.1)
        st[p + "attn.out_proj.weight"], st[p + "attn.out_proj.bias"] = n((D, D), g_w), n((D,), 0.1)
        ln(p + "ln_2", st)
        st[p + "mlp.c_fc.weight"], st[p + "mlp.c_fc.bias"] = n((F, D), g_w), n((F,), 0.1)
        st[p + "mlp.c_proj.weight"], st[p + "mlp.c_proj.bias"] = n((D, F), g_w), n((D,), 0.1)
    ln("visual.ln_post", st)
    st["visual.proj"] = n((D, E), g_w)
    return st


def to_transformers(st: dict) -> dict:
    """the same weights under the ``transformers`` key scheme (CLIPVisionModelWithProjection.state_dict), torch tensors"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    D = st["visual.conv1.weight"].shape[0]
    out = {"vision_model.embeddings.class_embedding": t(st["visual.class_embedding"]),
           "vision_model.embeddings.patch_embedding.weight": t(st["visual.conv1.weight"]),
           "vision_model.embeddings.position_embedding.weight": t(st["visual.positional_embedding"]),
           "vision_model.pre_layrnorm.weight": t(st["visual.ln_pre.weight"]), "vision_model.pre_layrnorm.bias": t(st["visual.ln_pre.bias"]),
           "vision_model.post_layernorm.weight": t(st["visual.ln_post.weight"]),
           "vision_model.post_layernorm.bias": t(st["visual.ln_post.bias"]),
           "visual_projection.weight": t(st["visual.proj"].T)}
    names = {"attn.out_proj": "self_attn.out_proj", "ln_1": "layer_norm1", "ln_2": "layer_norm2", "mlp.c_fc": "mlp.fc1",
             "mlp.c_proj": "mlp.fc2"}
    i = 0
    while f"visual.transformer.resblocks.{i}.ln_1.weight" in st:
        p, q = f"visual.transformer.resblocks.{i}.", f"vision_model.encoder.layers.{i}."
        for kind in ("weight", "bias"):
            w = st[p + "attn.in_proj_" + kind]
            for j, name in enumerate(("q_proj", "k_proj", "v_proj")):
                out[f"{q}self_attn.{name}.{kind}"] = t(w[j * D:(j + 1) * D])
            for a, b in names.items():
                out[f"{q}{b}.{kind}"] = t(st[f"{p}{a}.{kind}"])
        i += 1
    return out


# ---------------------------------------------------------------------------------------------------- image processor
def resized_size(width: int, height: int, size: int):
    short, long = (width, height) if width <= height else (height, width)
    new_long = int(size * long / short)
    return (size, new_long) if width <= height else (new_long, size)


def preprocess_u8(image, size: int = 224) -> np.ndarray:
    """PIL image -> the uint8 RGB clip (size, size, 3): convert RGB, BICUBIC shortest edge, centre crop"""
    from PIL import Image

    image = image.convert("RGB")
    w, h = image.size
    nw, nh = resized_size(w, h, size)
    if (nw, nh) != (w, h):
        image = image.resize((nw, nh), Image.BICUBIC)
    left, top = (nw - size) // 2, (nh - size) // 2
    return np.ascontiguousarray(np.asarray(image)[top:top + size, left:left + size])


def pixel_values(clips_rgb_u8: np.ndarray, dtype=torch.float32) -> torch.Tensor:
    """uint8 RGB clips (n, S, S, 3) -> (n, 3, S, S): x / 255, (x - mean) / std, in ``dtype``"""
    x = torch.from_numpy(np.ascontiguousarray(clips_rgb_u8)).to(dtype) / 255
    mean, std = torch.tensor(CLIP_MEAN, dtype=dtype), torch.tensor(CLIP_STD, dtype=dtype)
    return ((x - mean) / std).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------- the tower
def _ln(x, st, prefix, eps=1e-5):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), st[prefix + ".weight"], st[prefix + ".bias"], eps)


def forward(state: dict, cfg: dict, pixels: torch.Tensor, dtype=torch.float64):
    """-> (taps [depth + 1][n][tokens][D]: the residual stream after pre_layrnorm and after every layer, embeddings [n][E])"""
    st = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}
    D, H, P = cfg["dim"], cfg["heads"], cfg["patch"]
    x = pixels.to(dtype)
    n = x.shape[0]
    pe = torch.nn.functional.conv2d(x, st["visual.conv1.weight"], stride=P).flatten(2).transpose(1, 2)      # [n][np][D]
    h = torch.cat([st["visual.class_embedding"].expand(n, 1, D), pe], dim=1) + st["visual.positional_embedding"]
    h = _ln(h, st, "visual.ln_pre")
    taps = [h]
    T = h.shape[1]
    for i in range(cfg["depth"]):
        p = f"visual.transformer.resblocks.{i}."
        y = _ln(h, st, p + "ln_1")
        qkv = y @ st[p + "attn.in_proj_weight"].T + st[p + "attn.in_proj_bias"]
        q, k, v = (t.reshape(n, T, H, D // H).transpose(1, 2) for t in qkv.split(D, dim=-1))
        a = torch.softmax(q @ k.transpose(-1, -2) * (D // H) ** -0.5, dim=-1) @ v
        h = h + a.transpose(1, 2).reshape(n, T, D) @ st[p + "attn.out_proj.weight"].T + st[p + "attn.out_proj.bias"]
        y = _ln(h, st, p + "ln_2") @ st[p + "mlp.c_fc.weight"].T + st[p + "mlp.c_fc.bias"]
        y = y * torch.sigmoid(1.702 * y)
        h = h + y @ st[p + "mlp.c_proj.weight"].T + st[p + "mlp.c_proj.bias"]
        taps.append(h)
    emb = _ln(h[:, 0], st, "visual.ln_post") @ st["visual.proj"]
    return torch.stack(taps), emb


def cosine(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x . y / max(|x| |y|, 1e-8) over the last axis"""
    return (x * y).sum(-1) / torch.clamp(x.norm(dim=-1) * y.norm(dim=-1), min=1e-8)


def cosine_matrix(emb: torch.Tensor) -> torch.Tensor:
    return cosine(emb[:, None, :], emb[None, :, :])


# ---------------------------------------------------------------------------------------------------- the test clips
def make_clips(size: int = 224) -> np.ndarray:
    """eight RGB uint8 clips: uniform noise, all black, all white, a colour gradient, a 16-pixel checkerboard, dark boxes on
    white, its inverse, and the boxes image with one extra 10 x 30 black bar"""
    rng = np.random.default_rng(3)
    S = size
    noise = rng.integers(0, 256, (S, S, 3)).astype(np.uint8)
    black, white = np.zeros((S, S, 3), np.uint8), np.full((S, S, 3), 255, np.uint8)
    ramp = np.linspace(0, 255, S)
    grad = np.stack([np.broadcast_to(ramp[None, :], (S, S)), np.broadcast_to(ramp[:, None], (S, S)),
                     np.broadcast_to(ramp[::-1][None, :], (S, S))], axis=-1).astype(np.uint8)
    yy, xx = np.mgrid[0:S, 0:S]
    checker = np.repeat((((yy // 16 + xx // 16) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    boxes = white.copy()
    for x, y, w, h, shade in ((20, 30, 60, 18, 30), (100, 30, 90, 18, 60), (20, 80, 150, 12, 10), (40, 130, 50, 50, 90),
                              (130, 140, 70, 30, 40)):
        boxes[y:y + h, x:x + w] = shade
    bar = boxes.copy()
    bar[190:200, 150:180] = 0
    return np.stack([noise, black, white, grad, checker, boxes, 255 - boxes, bar])
