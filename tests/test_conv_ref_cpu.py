"""tests/conv_ref.py (the float64 tap-sum reference the GPU parity tests of conv_igemm use) against torch.nn.functional.conv2d /
max_pool2d in float64, at the shapes of the GPU cases (tests/conv_cases.py; the two 49 087-pixel maps are left to the GPU file),
and its concat and row-mapping helpers against torch.cat / explicit indexing.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import conv_ref as cr

SMALL = [c for c in cc.ALL if c["B"] * c["H"] * c["W"] < 40000]
U64 = 2.0 ** -53


def _torch_ref(c, ops):
    """the case through F.conv2d (NCHW, float64): -> unpooled activated map, pooled output, magnitude map, all NHWC"""
    x = ops["x"] if ops["x2"] is None else torch.cat([ops["x"], ops["x2"]], dim=3)
    x, w = x.double().permute(0, 3, 1, 2), ops["w"].double().permute(0, 3, 1, 2)
    px = c["pad"] if c["pad_x"] < 0 else c["pad_x"]
    kw = dict(stride=(c["sy"], 1), padding=(c["pad"], px), dilation=c["dil"])
    N = c["N"]
    s = torch.ones(N, dtype=torch.float64) if ops["scale"] is None else ops["scale"].double()
    b = ops["bias"].double()
    t = F.conv2d(x, w, **kw) * s[None, :, None, None] + b[None, :, None, None]
    mag = F.conv2d(x.abs(), w.abs(), **kw) * s.abs()[None, :, None, None] + b.abs()[None, :, None, None]
    if ops["res"] is not None:
        r = ops["res"].double()
        B, _, Ho, Wo = t.shape
        if c["period"]:
            r = torch.stack([r[q % c["period"]] for q in range(B * Ho * Wo)])
        r = r.reshape(B, Ho, Wo, N).permute(0, 3, 1, 2)
        t, mag = t + r, mag + r.abs()
    v = F.relu(t) if c["act"] == cc.RELU else (F.gelu(t) if c["act"] == cc.GELU else t)
    out = v
    if c["pool"] == cc.P22:
        out = F.max_pool2d(v, 2, 2)
    elif c["pool"] == cc.P21:
        out = F.max_pool2d(v, (2, 1), (2, 1))
    return tuple(a.permute(0, 2, 3, 1) for a in (v, out, mag))


def ref_of(c, ops):
    return cr.conv_ref(ops["x"], ops["w"], x2=ops["x2"], scale=ops["scale"], bias=ops["bias"], sy=c["sy"], pad=c["pad"],
                       pad_x=c["pad_x"], dil=c["dil"], act=c["act"], res=ops["res"], pool=c["pool"], row_period=c["period"])


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_reference_matches_torch(case):
    prec = "f32" if "f32" in case["precs"] else "f16"
    ops = cc.operands(case, prec)
    r = ref_of(case, ops)
    v, out, mag = _torch_ref(case, ops)
    Ho, Wo, Hp, Wp, _, _ = cc.geometry(case)
    assert r["v"].shape == (case["B"], Ho, Wo, case["N"]) and r["out"].shape == (case["B"], Hp, Wp, case["N"])
    assert r["out"].shape == out.shape
    K = case["KH"] * case["KW"] * cc.cin(case, prec)
    tol = 2 * (K + 8) * U64 * mag                      # two float64 sums of K products, in whatever order
    assert bool(((r["mag"] - mag).abs() <= tol).all())
    assert bool(((r["v"] - v).abs() <= tol).all())
    assert bool(((r["out"] - out).abs() <= cr.pool_max(tol, case["pool"])).all())


def test_concat_equals_the_concatenated_tensor():
    for case in cc.CONCAT:
        ops = cc.operands(case, "f32")
        cat = torch.cat([ops["x"], ops["x2"]], dim=3)
        assert ops["x"].shape[3] == case["Cin1"] and cat.shape[3] == case["Cin"]
        a = ref_of(case, ops)
        b = cr.conv_ref(cat, ops["w"], scale=ops["scale"], bias=ops["bias"], act=case["act"], pad=0)
        assert bool(((a["out"] - b["out"]).abs() <= 4 * case["Cin"] * U64 * a["mag"]).all())
        # the two halves in the wrong order give something else
        wrong = cr.conv_ref(torch.cat([ops["x2"], ops["x"]], dim=3), ops["w"], scale=ops["scale"], bias=ops["bias"], act=case["act"], pad=0)
        assert float((a["out"] - wrong["out"]).abs().max()) > 0.1


def test_row_mapping_and_ownership():
    for M, period, stride, off in ((150, 50, 50, 0), (150, 50, 53, 1), (150, 50, 50, 1), (7, 0, 0, 0)):
        rows = cr.out_rows(M, period, stride, off)
        want = [(q // period) * stride + off + q % period if period else q for q in range(M)]
        assert rows.tolist() == want and len(set(want)) == M
    rows = cr.out_rows(6, 3, 5, 1)                   # rows 1 2 3, 6 7 8 of 10
    for own, n_own in ((False, 13), (True, 16)):
        m = cr.owned(10, 24, rows, 13, own)
        for r in range(10):
            for col in range(24):
                assert bool(m[r, col]) == (r in (1, 2, 3, 6, 7, 8) and col < n_own)


def test_residual_is_added_before_the_relu_and_gelu_is_refused():
    case = cc.RESIDUAL[0]
    ops = cc.operands(case, "f32")
    r = ref_of(case, ops)
    res = ops["res"].double().reshape(r["t"].shape)
    assert bool((r["v"] == torch.clamp(r["t"] + res, min=0)).all())
    up, down = (r["t"] < 0) & (r["t"] + res > 0), (r["t"] > 0) & (r["t"] + res < 0)
    assert float(up.double().mean()) >= 0.05 and float(down.double().mean()) >= 0.05
    with pytest.raises(ValueError):
        cr.conv_ref(ops["x"], ops["w"], res=ops["res"], act=cr.ACT_GELU, pad=1)
    with pytest.raises(ValueError):
        cr.conv_ref(ops["x"], ops["w"], res=ops["res"], pool=cr.POOL_2x2, pad=1)


def test_pool_floor_drops_the_last_row_and_column():
    v = torch.arange(2 * 5 * 7 * 3, dtype=torch.float64).reshape(2, 5, 7, 3)
    v[:, 4] = 1e9                                    # the dropped row and column hold the largest values
    v[:, :, 6] = 1e9
    p = cr.pool_max(v, cr.POOL_2x2)
    assert p.shape == (2, 2, 3, 3) and float(p.max()) < 1e9
    assert bool((p == v[:, 1:4:2, 1:6:2]).all())     # increasing values: the window's last member
    q = cr.pool_max(v[:, :, :6], cr.POOL_2x1)
    assert q.shape == (2, 2, 6, 3) and bool((q == v[:, 1:4:2, :6]).all())
