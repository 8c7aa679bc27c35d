"""No GPU: what the kernel-level tests of csrc/icr_ops.hip and csrc/image_ops.hip (tests/test_icr_ops_gpu.py,
tests/test_image_ops_gpu.py) stand on.

(a) the numpy restatements in tests/icr_ops_ref.py are pinned: the TPS grid to the oracle's fp32 grid, the AttentionCell context
    and cell to a torch float64 AttentionCell built from the same weights;
(b) every input condition the GPU tests' bars assume holds on the float64 reference alone: O(1) outputs (largest |entry| in
    [0.5, 2]), the share of ReLU zeros, the share of clamped TPS samples, how sharp the soft-max is;
(c) every witness: each mistake a kernel of this kind is prone to, applied to the float64 reference, moves the output by at
    least 0.05 = 50 bars on the inputs the GPU test uses (any change, for the exact kernels) — so those inputs can tell a wrong
    kernel from a right one.
"""
import numpy as np
import pytest
import torch

import icr_ops_ref as R


def _o1(ref, tag):
    m = float(np.abs(ref).max())
    print(f"{tag}: largest |entry| {m:.3f}")
    assert 0.5 <= m <= 2.0, (tag, m)


def _moves(ref, wrong, tag, what):
    d = float(np.abs(np.asarray(ref, np.float64) - np.asarray(wrong, np.float64)).max())
    print(f"{tag}: {what} moves the reference by {d:.3f}")
    assert d >= R.WITNESS, (tag, what, d)


# ----------------------------------------------------------------------------------------------------------------- (a) pins
def test_tps_grid_matches_the_oracle():
    from marie_icr_amd.weights import make_icr_state
    from oracle.icr_torch import TorchIcrOracle

    orc = TorchIcrOracle(make_icr_state(0))
    inv, p_hat = R.tps_constants(20, 32, 100)
    st = orc.st
    assert np.abs(inv - st["Transformation.GridGenerator.inv_delta_C"].numpy()).max() <= 1e-4 * np.abs(inv).max()
    assert np.abs(p_hat - st["Transformation.GridGenerator.P_hat"].numpy()).max() <= 1e-5
    rng = np.random.default_rng(3)
    cp = (R.tps_fiducials(20)[None] + rng.uniform(-0.15, 0.15, size=(4, 20, 2))).astype(np.float32)
    got = R.tps_grid(cp, inv, p_hat)
    ref = orc.tps_grid(torch.from_numpy(cp)).numpy()
    err = float(np.abs(got - ref).max())
    print(f"TPS grid vs the oracle's fp32 grid: {err:.2e}")
    assert err <= 1e-4
    # the identity fiducials give the pixel centres back, for any F, H, W
    for Fn, H, W in ((6, 4, 6), (20, 32, 100), (8, 5, 3)):
        inv, p_hat = R.tps_constants(Fn, H, W)
        g = R.tps_grid(R.tps_fiducials(Fn)[None], inv, p_hat)[0]
        assert np.abs(g - p_hat[:, 1:3]).max() <= 1e-9


class _AttentionCell(torch.nn.Module):
    """AttentionCell (prediction.py:63-83) from torch's own modules, float64"""

    def __init__(self, nc):
        super().__init__()
        self.i2h = torch.nn.Linear(256, 256, bias=False)
        self.h2h = torch.nn.Linear(256, 256)
        self.score = torch.nn.Linear(256, 1, bias=False)
        self.rnn = torch.nn.LSTMCell(256 + nc, 256)

    def forward(self, h, c, batch_H, onehot):
        e = self.score(torch.tanh(self.i2h(batch_H) + self.h2h(h).unsqueeze(1)))
        alpha = torch.softmax(e, dim=1)
        context = torch.bmm(alpha.permute(0, 2, 1), batch_H).squeeze(1)
        h, c = self.rnn(torch.cat([context, onehot], 1), (h, c))
        return context, h, c


@pytest.mark.parametrize("T", [1, 26, 64])
def test_context_and_cell_match_a_torch_attention_cell(T):
    torch.manual_seed(5 + T)
    nc, B = R.NUM_CLASS, 3
    cell = _AttentionCell(nc).double()
    h, c = torch.randn(B, 256, dtype=torch.float64) * 0.5, torch.rand(B, 256, dtype=torch.float64) * 2 - 1
    batch_H = torch.randn(B, T, 256, dtype=torch.float64)
    chars = torch.tensor([0, 95, 41])
    with torch.no_grad():
        ctx_t, h_t, c_t = cell(h, c, batch_H, torch.nn.functional.one_hot(chars, nc).double())
        # the decomposition the kernels are fed (icr_api.hip): one GEMM row holds h2h(h) + bias | W_hh h + b_ih + b_hh
        hproj = cell.i2h(batch_H).numpy()
        hp = cell.h2h(h).numpy()
        ghid = (h @ cell.rnn.weight_hh.T + cell.rnn.bias_ih + cell.rnn.bias_hh).numpy()
        w_ih = cell.rnn.weight_ih.numpy()
    ctx = R.attn_context(hproj, hp, cell.score.weight.detach().numpy()[0], batch_H.numpy())
    assert np.abs(ctx - ctx_t.numpy()).max() <= 1e-12
    h_n, c_n = R.attn_cell(ctx @ w_ih[:, :256].T, ghid, w_ih[:, 256:].T, chars.numpy(), c.numpy())
    assert np.abs(h_n - h_t.numpy()).max() <= 1e-12 and np.abs(c_n - c_t.numpy()).max() <= 1e-12


def test_argmax_reference_is_torch_max():
    x = np.array([[1, 3, 3, 2], [-np.inf] * 4, [0, np.nan, 5, np.nan], [2, 1, 0, np.nan]], np.float32)
    assert R.argmax_rows(x, 4).tolist() == [1, 0, 1, 3]
    assert R.argmax_rows(x, 3).tolist() == [1, 0, 1, 0]


# ----------------------------------------------------------------------------------------------------- (b), (c) per kernel
@pytest.mark.parametrize("cid,kw", R.GRAY_CASES, ids=[c for c, _ in R.GRAY_CASES])
def test_conv_gray_first_inputs(cid, kw):
    c = R.gray_case(**kw)
    ref = R.conv_gray_first(c["img"], c["w"], c["scale"], c["bias"])
    _o1(ref, cid)
    zeros = float((ref[..., :kw["C"]] == 0).mean())
    print(f"{cid}: ReLU zeros {zeros:.2f}")
    assert 0.10 <= zeros <= 0.90
    assert (ref[..., kw["C"]:] == 0).all()
    if kw["u8"]:
        assert (c["img"][:, 0, 0] == 0).all() and (c["img"][:, -1, -1] == 255).all()
    _moves(ref, R.conv_gray_first(c["img"], c["w"], c["scale"], c["bias"], taps_transposed=True), cid, "dy <-> dx")
    _moves(ref, R.conv_gray_first(c["img"], c["w"], c["scale"], c["bias"], pad_u8_zero=True), cid, "border = u8 0")


@pytest.mark.parametrize("cid,shape,neg,_p", R.S21_CASES, ids=[c[0] for c in R.S21_CASES])
def test_maxpool_s21_inputs(cid, shape, neg, _p):
    x = R.pool_input(61, shape, neg)
    assert (x < 0).all() if neg else ((x < 0).any() and (x > 0).any())
    ref = R.maxpool_s21_p01(x)
    assert ref.shape == (shape[0], shape[1] // 2, shape[2] + 1, shape[3])
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    assert not np.array_equal(ref, R.maxpool_s21_p01(x, pad_zero=True)), "padding = 0 goes unnoticed"
    if neg:
        assert (R.maxpool_s21_p01(x, pad_zero=True)[:, :, [0, -1]] == 0).all()


@pytest.mark.parametrize("cid,k,shape,neg,_p", R.MAXPOOL_CASES[:-1], ids=[c[0] for c in R.MAXPOOL_CASES[:-1]])
def test_maxpool_inputs(cid, k, shape, neg, _p):
    x = R.pool_input(67, shape, neg)
    assert (x < 0).all() if neg else ((x < 0).any() and (x > 0).any())
    ref = R.maxpool(x, k)
    assert ref.shape[1:3] == ((shape[1] // 2, shape[2] // 2) if k == 2 else shape[1:3])
    if k == 3:
        assert not np.array_equal(ref, R.maxpool(x, 3, pad_zero=True)), "padding = 0 goes unnoticed"


def test_maxpool_negative_cases():
    assert sum(c[3] for c in R.MAXPOOL_CASES) == 2 and sum(c[2] for c in R.S21_CASES) >= 1


@pytest.mark.parametrize("shape", R.AVG_SHAPES, ids=str)
def test_avgpool_inputs(shape):
    ref = R.avgpool_hw(R.avg_input(71, shape))
    _o1(ref, f"avgpool {shape}")


@pytest.mark.parametrize("cid,kw", R.TPS_CASES, ids=[c for c, _ in R.TPS_CASES])
def test_tps_inputs(cid, kw):
    c = R.tps_case(**kw)
    n = R.norm_u8(c["crops"])
    step = max(float(np.abs(np.diff(n, axis=1)).max()), float(np.abs(np.diff(n, axis=2)).max()))
    print(f"{cid}: largest neighbour difference {step:.3f}")
    assert step <= 0.1
    if kw["H"] == 32:
        assert c["crops"][0, 0, 0] == 0 and c["crops"][0, -1, -1] == 255
    args = (c["crops"], c["c_prime"], c["inv_delta_c"], c["p_hat"])
    ref = R.tps_sample(*args)
    _o1(ref, cid)
    clamp = R.tps_clamped(*args[1:])
    share = float(clamp.any(-1).mean())
    print(f"{cid}: clamped samples {share:.2f}")
    if kw["kind"] == "identity":
        # the identity fiducials give the crop back as grid_sample reads pixel centres with align_corners=True (R.tps_identity_expected)
        assert share == 0 and np.abs(ref - R.tps_identity_expected(c["crops"])).max() <= 1e-4
    if kw["kind"] == "jitter" and kw["B"] > 1:
        assert not np.array_equal(c["c_prime"][0], c["c_prime"][1])
    if kw["kind"] == "x1.5":
        assert share >= 0.10 and clamp.any(axis=(0, 1)).all(), (share, clamp.any(axis=(0, 1)))
        _moves(ref, R.tps_sample(*args, padding_mode="zeros"), cid, "zero padding")
    if kw["kind"] != "x1.5":       # on (c) most samples are clamped either way; what is left moves by under half a pixel
        _moves(ref, R.tps_sample(*args, align_corners=False), cid, "align_corners=False")
    if kw["B"] > 1:
        _moves(ref, R.tps_sample(*args, ignore_b=True), cid, "image index without b")


@pytest.mark.parametrize("cid,kw", R.ATTN_CONTEXT_CASES, ids=[c for c, _ in R.ATTN_CONTEXT_CASES])
def test_attn_context_inputs(cid, kw):
    c = R.attn_context_case(**kw)
    assert np.isnan(c["hp"][:, 256:]).all() and np.isfinite(c["hp"][:, :256]).all()
    assert np.array_equal(R.f16(c["H"]), c["H"])
    ref = R.attn_context(c["hproj"], c["hp"][:, :256], c["score_w"], c["H"])
    _o1(ref, cid)
    top = R.attn_alpha(R.attn_scores(c["hproj"], c["hp"][:, :256], c["score_w"])).max(axis=1)
    print(f"{cid}: largest probability mean {top.mean():.3f} max {top.max():.3f}")
    if kw["T"] < 64 and not kw["sharp"]:      # flat rows: 64 - T slots of weight exp(0 - max) are a large share of the sum
        _moves(ref, R.attn_context(c["hproj"], c["hp"][:, :256], c["score_w"], c["H"], softmax_over_64=True), cid,
               "soft-max over 64 slots")


def test_attn_context_sharpness():
    """over all the T = 26 rows of the flat and of the sharp cases (score_w x 8)"""
    tops = {False: [], True: []}
    for _, kw in R.ATTN_CONTEXT_CASES:
        if kw["T"] == 26:
            c = R.attn_context_case(**kw)
            tops[kw["sharp"]] += list(R.attn_alpha(R.attn_scores(c["hproj"], c["hp"][:, :256], c["score_w"])).max(axis=1))
    flat, sharp = np.array(tops[False]), np.array(tops[True])
    print(f"flat: mean top probability {flat.mean():.3f}; sharp: mean {sharp.mean():.3f} max {sharp.max():.3f}")
    assert flat.mean() < 0.3
    assert sharp.mean() > 0.6 and sharp.max() > 0.9


@pytest.mark.parametrize("B", [1, 3])
def test_attn_cell_inputs(B):
    c = R.attn_cell_case(B)
    assert np.isnan(c["ghid"][:, :256]).all() and np.abs(c["c_prev"]).max() <= 1
    assert (95 in c["chars"]) and (B == 1 or (0 in c["chars"] and len(set(c["chars"].tolist())) == B))
    pre = c["gctx"].astype(np.float64) + c["ghid"][:, 256:] + c["w_onehot"][c["chars"]]
    big = np.abs(pre) > 50
    print(f"attn_cell B{B}: pre-activation std {pre[~big].std():.2f}, {int(big.sum())} entries near +-100")
    assert 1.2 <= pre[~big].std() <= 1.6 and big.sum() >= 4 and (pre[big] > 0).any() and (pre[big] < 0).any()
    args = (c["gctx"], c["ghid"][:, 256:], c["w_onehot"], c["chars"], c["c_prev"])
    h, cn = R.attn_cell(*args)
    assert np.isfinite(h).all() and np.isfinite(cn).all()
    _o1(h, f"attn_cell B{B} h")
    _o1(cn, f"attn_cell B{B} c")
    for name, wrong in (("gate order i, g, f, o", R.attn_cell(*args, gate_order="igfo")),
                        ("one-hot row of chars[0]", R.attn_cell(*args, chars_from_row0=True) if B > 1 else None)):
        if wrong is not None:
            _moves(h, wrong[0], f"attn_cell B{B} h", name)
            _moves(cn, wrong[1], f"attn_cell B{B} c", name)


@pytest.mark.parametrize("C", R.ARGMAX_C)
def test_argmax_inputs(C):
    rows, names, first_nf = R.argmax_rows_case(C)
    ref = R.argmax_rows(rows, C)
    assert ((ref >= 0) & (ref < C)).all()
    for r, name, i in zip(rows, names, ref):
        if name.startswith("tie"):
            hits = np.flatnonzero(r == r.max())
            assert len(hits) == 2 and i == hits[0], (name, hits, i)
            assert (hits[0] % 64 == hits[1] % 64) == (name == "tie-lane")
        if name == "all-minus-inf":
            assert i == 0
        if name == "nan-last":
            assert i == C - 1
        if name == "nan-3-70":
            assert i == 3 and r[1] == 9.0
        if name == "span":
            x = r.astype(np.float64)
            t = np.exp(x - x.max())            # most terms vanish against the largest in fp32, a good share below its smallest normal
            assert C < 64 or ((t < 2.0 ** -24).mean() > 0.5 and (t < 2.0 ** -126).mean() > 0.1)
    assert names.index("all-minus-inf") == first_nf
    if C == 1:
        assert (R.softmax_pmax(rows[:first_nf]) == 1.0).all()
    # witness (exact kernel): a last-maximum rule, or a NaN-blind one, gives another index on these rows
    last = np.array([C - 1 - int(np.nanargmax(r[::-1])) if np.isfinite(r).any() else C - 1 for r in rows])
    assert C == 1 or (last != ref).any()


@pytest.mark.parametrize("th,tw,H,W", R.RGB_SHAPES, ids=str)
def test_conv_rgb_first_inputs(th, tw, H, W):
    c = R.rgb_case(th, tw, H, W)
    args = (c["img"], H, W, c["w"], c["scale"], c["bias"])
    ref = R.conv_rgb_first(*args)
    _o1(ref, f"conv_rgb {th}x{tw}")
    zeros = float((ref == 0).mean())
    assert 0.10 <= zeros <= 0.90, zeros
    means = c["img"].reshape(-1, 3).mean(0)
    assert means[0] > 1.3 * means[1] > 1.3 * 1.3 * means[2]
    _moves(ref, R.conv_rgb_first(*args, channels_reversed=True), f"conv_rgb {th}x{tw}", "channel order reversed")
    if (th, tw) != (H, W):
        _moves(ref, R.conv_rgb_first(*args, canvas_pad_zero=True), f"conv_rgb {th}x{tw}", "canvas padding 0 after normalisation")
    e_ref = float(np.abs(R.conv_rgb_first(*args, f16_emulated=True) - ref).max())
    print(f"conv_rgb {th}x{tw}: E_ref {e_ref:.2e}")
    assert 1e-4 <= e_ref <= 1e-2                       # a rounding-level figure: the f16 bar 2 * E_ref is no free pass
    assert -(-(H * W) // 16) > 4 * 4096 or H < 520     # the last case: more 16-pixel tiles than the MFMA launch has waves


@pytest.mark.parametrize("cid,shape,size,_p", R.UPSAMPLE_CASES[:-1], ids=[c[0] for c in R.UPSAMPLE_CASES[:-1]])
def test_upsample_inputs(cid, shape, size, _p):
    x = R.upsample_input(73, shape)
    ref = R.upsample_bilinear(x, *size)
    _o1(ref, cid)
    if shape[1] > 1:
        _moves(ref, R.upsample_bilinear(x, *size, align_corners=True), cid, "align_corners=True")


@pytest.mark.parametrize("cid,stride,npix,_p", R.SCORE_CASES, ids=[c[0] for c in R.SCORE_CASES])
def test_score_head_inputs(cid, stride, npix, _p):
    c = R.score_case(stride, npix)
    assert (stride == 16 or np.isnan(c["x"][:, 16:]).all()) and np.array_equal(R.f16(c["x"][:, :16]), c["x"][:, :16])
    args = (c["x"][:, :16], c["w1"], c["b1"], c["w2"], c["b2"])
    ref = R.score_head(*args)
    _o1(ref, cid)
    hidden = c["x"][:, :16].astype(np.float64) @ c["w1"].astype(np.float64).T + c["b1"]
    cut = float((hidden <= 0).mean())
    print(f"{cid}: the hidden ReLU cuts {cut:.2f}")
    assert 0.10 <= cut <= 0.90
    _moves(ref, R.score_head(*args, w2_rows_swapped=True), cid, "w2 rows swapped")
    _moves(ref, R.score_head(*args, no_relu=True), cid, "no hidden ReLU")
    e_ref = float(np.abs(R.score_head(*args, f16_emulated=True) - ref).max())
    print(f"{cid}: E_ref {e_ref:.2e}")
    assert 0 < e_ref <= 5e-3


@pytest.mark.parametrize("src,dst", R.RESIZE_CASES, ids=str)
def test_resize_reference_shapes(src, dst):
    img = np.random.default_rng(79).integers(0, 256, size=src + (3,)).astype(np.uint8)
    out = R.resize_linear_u8(img, *dst)
    assert out.shape == dst + (3,) and out.dtype == np.uint8
    if src == dst:
        assert np.array_equal(out, img)
