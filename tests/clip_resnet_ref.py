"""Plain-torch restatement of CLIP's ModifiedResNet vision tower (clip/model.py: ModifiedResNet, Bottleneck, AttentionPool2d),
parameterised by dtype, plus the seeded weights the tests use (test infrastructure: the GPU tests compare the HIP model
against it).  The ``clip`` package is not installed, so nothing pins this file to the library: tests/test_clip_resnet_cpu.py
checks it in float64 against an independently written numpy attention pool and a per-block computation instead.

Weights are taken under the OpenAI key scheme (``visual.*``), which is what marie_icr_amd.embeddings.load_clip_resnet_state
stages.  The image processor and the test clips are tests/clip_ref.py's.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

SMALL = dict(width=16, layers=(1, 2, 1, 1), image_size=64, proj_dim=64)          # 5 tokens; channels 8 .. 512, most of them padded
SMALL_96 = dict(SMALL, image_size=96)                                             # 10 tokens
RN50X4 = dict(width=80, layers=(4, 6, 10, 6), image_size=288, proj_dim=640)      # 82 tokens
RN50 = dict(width=64, layers=(3, 4, 6, 3), image_size=224, proj_dim=1024)
RN101 = dict(width=64, layers=(3, 4, 23, 3), image_size=224, proj_dim=512)
# the gains of the seeded recipe: (factor on bn3.weight, shift of the bn3 / downsample.1 biases).  The shift makes the blocks'
# ReLUs cut; too large a shift kills the network (every cosine becomes 1: with this recipe's running statistics -0.5 already
# does), none lets RN50x4's 26 blocks grow the maps past 100.  Measured on the CPU restatement in fp32 over the eight clips of
# clip_ref.make_clips() resized to the model's size: cosines 0.25 .. 1.0000 / 0.16 .. 0.9999 / 0.13 .. 0.9999, largest
# embedding entry 1.45 / 1.19 / 4.06, largest tap entries 5.8 .. 12.9 / 9.0 .. 14.0 / 10.0 .. 17.2
GAINS = {"small": (0.3, -0.25), "small_96": (0.3, -0.25), "rn50x4": (0.3, -0.3)}
BN_EPS = 1e-5


def blocks(cfg: dict):
    """(key prefix, input channels, planes, stride, has a downsample path) of every Bottleneck, in order"""
    out, cin = [], cfg["width"]
    for l in range(4):
        planes = cfg["width"] << l
        for i in range(cfg["layers"][l]):
            stride = 2 if (i == 0 and l > 0) else 1
            out.append((f"visual.layer{l + 1}.{i}.", cin, planes, stride, stride > 1 or cin != 4 * planes))
            cin = 4 * planes
    return out


def n_tokens(cfg: dict) -> int:
    return (cfg["image_size"] // 32) ** 2 + 1


def make_state(cfg: dict, gains, seed: int = 0, zeros: bool = False) -> dict:
    """seeded OpenAI-scheme weights (float32 arrays): He-initialised convolutions, BatchNorm gains 1 + 0.1 N (bn3: times
    gains[0]), biases 0.1 N (bn3 and downsample.1: plus gains[1]), running means 0.1 N, running variances U(0.5, 1.5); the
    attention pool as clip initialises it (N(0, embed_dim^-0.5)) with biases 0.1 N.  ``zeros``: tensors of the right shapes
    filled with zeros (the loader's geometry tests)"""
    rng = np.random.default_rng(seed)
    w, E, P = cfg["width"], 32 * cfg["width"], cfg["proj_dim"]
    st = {}

    def n(shape, s):
        return np.zeros(shape, np.float32) if zeros else (rng.standard_normal(shape) * s).astype(np.float32)

    def conv_bn(conv, bn, co, ci, k, gain=1.0, shift=0.0):
        st[conv + ".weight"] = n((co, ci, k, k), (2.0 / (ci * k * k)) ** 0.5)
        st[bn + ".weight"] = (gain * (1.0 + n((co,), 0.1))).astype(np.float32)
        st[bn + ".bias"] = (n((co,), 0.1) + shift).astype(np.float32)
        st[bn + ".running_mean"] = n((co,), 0.1)
        st[bn + ".running_var"] = np.ones(co, np.float32) if zeros else rng.uniform(0.5, 1.5, co).astype(np.float32)
        st[bn + ".num_batches_tracked"] = np.zeros((), np.float32)

    conv_bn("visual.conv1", "visual.bn1", w // 2, 3, 3)
    conv_bn("visual.conv2", "visual.bn2", w // 2, w // 2, 3)
    conv_bn("visual.conv3", "visual.bn3", w, w // 2, 3)
    for p, cin, planes, stride, down in blocks(cfg):
        conv_bn(p + "conv1", p + "bn1", planes, cin, 1)
        conv_bn(p + "conv2", p + "bn2", planes, planes, 3)
        conv_bn(p + "conv3", p + "bn3", 4 * planes, planes, 1, gains[0], gains[1])
        if down:
            conv_bn(p + "downsample.0", p + "downsample.1", 4 * planes, cin, 1, 1.0, gains[1])
    a = "visual.attnpool."
    st[a + "positional_embedding"] = n((n_tokens(cfg), E), E ** -0.5)
    for name in "qkv":
        st[a + name + "_proj.weight"], st[a + name + "_proj.bias"] = n((E, E), E ** -0.5), n((E,), 0.1)
    st[a + "c_proj.weight"], st[a + "c_proj.bias"] = n((P, E), E ** -0.5), n((P,), 0.1)
    return st


# ---------------------------------------------------------------------------------------------------- the tower
def _bn(x, st, p):
    return F.batch_norm(x, st[p + ".running_mean"], st[p + ".running_var"], st[p + ".weight"], st[p + ".bias"], False, 0.0, BN_EPS)


def bottleneck(st: dict, p: str, x: torch.Tensor, stride: int, down: bool) -> torch.Tensor:
    out = F.relu(_bn(F.conv2d(x, st[p + "conv1.weight"]), st, p + "bn1"))
    out = F.relu(_bn(F.conv2d(out, st[p + "conv2.weight"], padding=1), st, p + "bn2"))
    if stride > 1:
        out = F.avg_pool2d(out, stride)
    out = _bn(F.conv2d(out, st[p + "conv3.weight"]), st, p + "bn3")
    identity = x
    if down:
        if stride > 1:
            identity = F.avg_pool2d(identity, stride)
        identity = _bn(F.conv2d(identity, st[p + "downsample.0.weight"]), st, p + "downsample.1")
    return F.relu(out + identity)


def attnpool(st: dict, x: torch.Tensor, heads: int) -> torch.Tensor:
    """AttentionPool2d.forward: x [n][E][H][W] -> [n][proj_dim]"""
    a = "visual.attnpool."
    x = x.flatten(start_dim=2).permute(2, 0, 1)                       # [HW][n][E]
    x = torch.cat([x.mean(dim=0, keepdim=True), x], dim=0)
    x = x + st[a + "positional_embedding"][:, None, :]
    out, _ = F.multi_head_attention_forward(
        query=x[:1], key=x, value=x, embed_dim_to_check=x.shape[-1], num_heads=heads,
        q_proj_weight=st[a + "q_proj.weight"], k_proj_weight=st[a + "k_proj.weight"], v_proj_weight=st[a + "v_proj.weight"],
        in_proj_weight=None, in_proj_bias=torch.cat([st[a + "q_proj.bias"], st[a + "k_proj.bias"], st[a + "v_proj.bias"]]),
        bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=st[a + "c_proj.weight"],
        out_proj_bias=st[a + "c_proj.bias"], use_separate_proj_weight=True, training=False, need_weights=False)
    return out.squeeze(0)


def forward(state: dict, cfg: dict, pixels: torch.Tensor, dtype=torch.float64):
    """pixels [n][3][S][S] -> (taps: the stem after its pool and the output of each of the four layers, NHWC [n][H][W][C];
    embeddings [n][proj_dim])"""
    st = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}
    x = pixels.to(dtype)
    x = F.relu(_bn(F.conv2d(x, st["visual.conv1.weight"], stride=2, padding=1), st, "visual.bn1"))
    x = F.relu(_bn(F.conv2d(x, st["visual.conv2.weight"], padding=1), st, "visual.bn2"))
    x = F.relu(_bn(F.conv2d(x, st["visual.conv3.weight"], padding=1), st, "visual.bn3"))
    x = F.avg_pool2d(x, 2)
    taps = [x.permute(0, 2, 3, 1).contiguous()]
    bl = blocks(cfg)
    for i, (p, cin, planes, stride, down) in enumerate(bl):
        x = bottleneck(st, p, x, stride, down)
        if i + 1 == len(bl) or bl[i + 1][0].split(".")[1] != p.split(".")[1]:
            taps.append(x.permute(0, 2, 3, 1).contiguous())
    return taps, attnpool(st, x, cfg["width"] * 32 // 64)
