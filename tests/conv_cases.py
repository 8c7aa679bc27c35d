"""The case tables of tests/test_conv_paths_gpu.py (conv_igemm's plain epilogue through mhip_conv2d_nhwc_ex) and their seeded
operands.  Kept apart from the GPU file so that tests/test_conv_ref_cpu.py can hold the float64 reference against torch at the
same shapes without a GPU.

A case is a dict: B, H, W, `cs` (input channels in K slices of 64 f16 / 32 f32 channels; `Cin` where both precisions take the
same count), KH, KW, pad, pad_x (-1 = pad), sy, dil, N, pool, act, out_f32, Cin1 (> 0: two input tensors), ldc, own (pad columns
of a pitched row are the call's), res (0 none, 1 residual), res_shift (bytes the residual pointer is moved off 16-byte alignment),
period / row_stride / row_offset, scale (0: no scale vector), neg (negative-heavy pre-activations), precs, and `tile`: the kernel
the launcher's rule picks, asserted from the launch profile."""
import math
import zlib

import torch

T64, T128, T256, S128 = "conv_igemm<64>", "conv_igemm<128>", "conv_igemm<256>", "conv_igemm<1128>"
NONE, RELU, GELU = 0, 1, 2
P0, P22, P21 = 0, 1, 2
SLICE = {"f16": 64, "f32": 32}
DTYPE = {"f16": torch.float16, "f32": torch.float32}

_DEFAULTS = dict(B=2, H=1, W=1, cs=1, Cin=None, KH=3, KW=3, pad=1, pad_x=-1, sy=1, dil=1, N=128, pool=P0, act=NONE, out_f32=0,
                 Cin1=0, ldc=0, own=0, res=0, res_shift=0, period=0, row_stride=0, row_offset=0, scale=1, neg=0,
                 precs=("f16", "f32"))


def _c(name, tile, **kw):
    assert not set(kw) - set(_DEFAULTS), set(kw) - set(_DEFAULTS)
    return dict(_DEFAULTS, name=name, tile=tile, **kw)


# ---- border taps: maps smaller than, equal to and just larger than the filter's reach; B = 2 so that a tap let across an image
# boundary reads the neighbour's (never zero) pixels
BORDER = [_c(f"border/3x3/H{H}W{W}", T64, H=H, W=W, N=64) for H in (1, 2, 5) for W in (1, 3, 7)]
BORDER += [_c(f"border/2x2/H{H}W{W}", S128, H=H, W=W, KH=2, KW=2, pad=0, cs=2, N=72, act=RELU) for H in (2, 5) for W in (3, 7)]
BORDER += [_c(f"border/dil6/H{H}W{W}", S128, H=H, W=W, pad=6, dil=6, N=72, act=GELU) for H, W in ((1, 1), (2, 7), (5, 3), (13, 13), (14, 14))]

# ---- pooling: Ho = 13, Wo = 23 odd (the floor drops a row / column), 792 / 828 rows = more than one tile and no multiple of one;
# no ReLU and pre-activations around -1, so a max that starts from 0 or misses a window member shows
POOL = [_c(f"pool/{'2x2' if p == P22 else '2x1'}/N{N}", tile, B=3, H=13, W=23, cs=cs, N=N, pool=p, neg=1)
        for p in (P22, P21) for N, cs, tile in ((64, 1, T64), (128, 2, T128), (192, 1, T256))]
# vertical stride with pooling (no caller; the kernel decodes the pooled row order to conv-output rows before it applies the stride)
POOL += [_c(f"pool/{'2x2' if p == P22 else '2x1'}/sy2", T128, H=13, W=10, sy=2, N=128, pool=p, neg=1) for p in (P22, P21)]

# ---- vertical stride, asymmetric padding: the attention recognizer's conv4_1 / conv4_2 and the overlay generator's strided 3x3
STRIDE = [
    _c("stride/icr_conv4_1", S128, H=4, W=6, KH=2, KW=2, sy=2, pad=0, pad_x=1, cs=2, N=72, act=RELU),
    _c("stride/icr_conv4_2", S128, H=2, W=7, KH=2, KW=2, pad=0, pad_x=0, cs=2, N=72, act=RELU),
    _c("stride/overlay_3x3_s2", S128, H=7, W=6, sy=2, N=128, scale=0),               # Ho = 6 / 2 + 1 = 4
    _c("stride/2x2_s2_oddH", S128, H=5, W=6, KH=2, KW=2, sy=2, pad=0, pad_x=1, N=72, act=RELU),   # Ho = 3 / 2 + 1: truncates
    _c("stride/3x3_s2_evenH", T64, H=6, W=5, sy=2, N=64),                                          # Ho = 5 / 2 + 1: truncates
]

# ---- residual, added before the ReLU
_RES = dict(H=6, W=11, act=RELU, res=1)
RESIDUAL = [
    _c("res/out_elem", S128, **_RES),
    _c("res/out_f32", S128, out_f32=1, **_RES),
    _c("res/ldc136", S128, ldc=136, **_RES),
    _c("res/N44_ldc48", T64, N=44, ldc=48, **_RES),                 # N % 8 != 0: the element-wise path handles the residual
    _c("res/shift8", S128, res_shift=8, **_RES),                    # the unaligned branch of `vec`
]

# ---- pitched rows with a ragged N: the pad columns [N, roundup(N, 8)) are the call's own (zeroed) or somebody else's (untouched)
_PITCH = dict(H=6, W=11, act=RELU)
PITCH = [
    _c("pitch/N45_ldc48_own", T64, N=45, ldc=48, own=1, **_PITCH),
    _c("pitch/N45_ldc96", T64, N=45, ldc=96, **_PITCH),
    _c("pitch/N77_ldc80_own", S128, N=77, ldc=80, own=1, **_PITCH),
    _c("pitch/N77_ldc88", S128, N=77, ldc=88, **_PITCH),
]

# ---- periodic output rows (the fp32 / f16 patch embeddings): 3 images of np rows, residual of np rows
_PER = dict(B=1, H=1, KH=1, KW=1, pad=0, cs=3, res=1)
PERIOD = [_c(f"period/np50/stride{st}/off{off}", S128, W=150, period=50, row_stride=st, row_offset=off, act=act, **_PER)
          for st, off, act in ((50, 0, NONE), (50, 1, RELU), (53, 0, RELU), (53, 1, NONE))]
PERIOD += [_c("period/np16400/stride16403/off1", T128, W=3 * 16400, period=16400, row_stride=16403, row_offset=1, **dict(_PER, cs=1))]

# ---- 1x1 conv over two tensors
_CAT = dict(H=9, W=11, KH=1, KW=1, pad=0, act=RELU)
CONCAT = [
    _c("concat/64of128/N64", T64, Cin=128, Cin1=64, N=64, **_CAT),
    _c("concat/128of192/N128", T128, Cin=192, Cin1=128, N=128, **_CAT),
    _c("concat/64of256/N192", T256, Cin=256, Cin1=64, N=192, **dict(_CAT, act=GELU)),
    _c("concat/128of256/N72", T128, Cin=256, Cin1=128, N=72, **_CAT),
]

# ---- unpooled spatial convs on the big tiles: 191 x 257 = 49 087 pixels = 192 tiles of 256 rows, the last one with 191
BIG = [
    _c("big/3x3/N128", T128, B=1, H=191, W=257, N=128, act=RELU),
    _c("big/3x3/N256", T256, B=1, H=191, W=257, N=256, act=RELU),
    # N > 128, 24 x 4 tiles of 256 columns < 192 <= 24 x 8 tiles of 128: the mid-tile rule
    _c("big/mid_tile/M6144/N1024", T128, B=6144, KH=1, KW=1, pad=0, N=1024, act=GELU),
]

# ---- the `pure` switch of a 1x1 GEMM: K * sizeof(T) + 128 <= 65536 walks pointers, beyond it the general gather runs
PURE = [_c(f"pure/{what}/{p}/K{K}", S128, B=130, KH=1, KW=1, pad=0, Cin=K, N=72, precs=(p,))
        for what, p, K in (("last_fast", "f16", 32704), ("first_general", "f16", 32768), ("last_fast", "f32", 16352), ("first_general", "f32", 16384))]

GROUPS = {"border": BORDER, "pool": POOL, "stride": STRIDE, "residual": RESIDUAL, "pitch": PITCH, "period": PERIOD, "concat": CONCAT, "big": BIG,
          "pure": PURE}
ALL = [c for g in GROUPS.values() for c in g]
assert len({c["name"] for c in ALL}) == len(ALL)

# ---- straight-line and bounds-checked copies (f16): the unpooled 3x3 conv on a map of H rows, one row shorter, one row taller.
# W and H are such that the shorter map ends W' > W rows into a tile which the map of H rows fills: the rows of that tile above the
# shorter map's last row are written by `body` there and by `f16_fast` here.  (The same cannot hold for the taller map as well: its
# shared rows come from the same copy, at another distance from the end of the grid.)
PAIRS = [
    # N, W, H, tile, rows per tile
    (64, 300, 4, T64, 512), (128, 100, 6, S128, 128), (128, 200, 248, T128, 256), (256, 200, 248, T256, 256),
]


def pair_case(N, W, H, tile):
    return _c(f"pair/N{N}/W{W}/H{H}", tile, B=1, H=H, W=W, N=N, act=RELU, precs=("f16",))


def cin(case, prec):
    return case["Cin"] or case["cs"] * SLICE[prec]


def geometry(case):
    """-> Ho, Wo, Hp, Wp, M (the GEMM rows the kernel enumerates, before pooling), rows (output pixels)"""
    c = case
    px = c["pad"] if c["pad_x"] < 0 else c["pad_x"]
    Ho = (c["H"] + 2 * c["pad"] - c["dil"] * (c["KH"] - 1) - 1) // c["sy"] + 1
    Wo = c["W"] + 2 * px - c["dil"] * (c["KW"] - 1)
    Hp, Wp = (Ho // 2 if c["pool"] else Ho), (Wo // 2 if c["pool"] == P22 else Wo)
    rows = c["B"] * Hp * Wp
    return Ho, Wo, Hp, Wp, rows * {P0: 1, P22: 4, P21: 2}[c["pool"]], rows


def _noise(g, *shape):
    return torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1


def operands(case, prec, H=None):
    """seeded operands on the host, rounded to the element types the device gets: x (, x2), w in `prec`; scale, bias fp32; the
    residual in the output's type.  `H` overrides the map's height (the pair tests draw the tallest map once and slice it)."""
    c = dict(case, H=H or case["H"])
    g = torch.Generator().manual_seed(zlib.crc32(f"{case['name']}/{prec}".encode()))
    dt = DTYPE[prec]
    Cin, N = cin(c, prec), c["N"]
    K = c["KH"] * c["KW"] * Cin
    x = _noise(g, c["B"], c["H"], c["W"], Cin).to(dt)
    w = (_noise(g, N, c["KH"], c["KW"], Cin) * math.sqrt(3.0 / K)).to(dt)
    ops = {"x": x, "w": w, "x2": None, "scale": None, "res": None}
    if c["Cin1"]:
        ops["x"], ops["x2"] = x[..., :c["Cin1"]].contiguous(), x[..., c["Cin1"]:].contiguous()
    if c["scale"]:
        s = 0.5 + torch.rand((N,), generator=g)
        ops["scale"] = torch.where(torch.rand((N,), generator=g) < 0.25, -s, s)           # a quarter of the channels negated
    ops["bias"] = _noise(g, N) * 0.5 - (1.0 if c["neg"] else 0.0)
    if c["res"]:
        Ho, Wo, _, _, _, rows = geometry(c)
        odt = torch.float32 if c["out_f32"] else dt
        r = _noise(g, c["period"] or rows, N) * 1.5
        if c["period"]:
            r += (torch.arange(c["period"], dtype=torch.float32) % 7)[:, None] * 0.25      # a pattern of its own per row
        ops["res"] = r.to(odt)
    return ops
