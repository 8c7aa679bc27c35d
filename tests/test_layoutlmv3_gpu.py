"""GPU parity of the LayoutLMv3 page classifier through the C ABI: the fp32 mode against the fp32 torch restatement at full
size, the biased attention kernel alone against an fp64 evaluation of its formula, the f16 mode under the margin rule, and
batch independence of ``predict``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layoutlmv3_ref as R  # noqa: E402

from marie_icr_amd.document_classifier import ByteLevelBPE, TransformersDocumentClassifier  # noqa: E402
from marie_icr_amd.weights import make_layoutlmv3_state, make_page_bgr, write_synthetic_bpe  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_BAR = 1e-3                 # the project's standing fp32 bar
FP32_ATTN_BAR = 1e-5            # the fp32 attention kernel alone, relative to the largest output
# The f16 bounds are 2 x the maxima measured once on an MI355X against the references named beside them (the factor 2 covers the
# run-to-run and seed-to-seed spread of a rounding-error maximum); the measurements are recorded in DESIGN.md §3 / §0.
F16_ATTN_ERR_MEASURED = 4.64e-4     # attn_flash_f16_kernel<BiasArgs> (the biased instance, attn_flash.hip) vs fp64, relative to the largest output, max over the six cases below
F16_ATTN_BOUND = 2 * F16_ATTN_ERR_MEASURED
F16_LOGIT_ERR_MEASURED = 6.29e-2    # f16 model logits vs the fp32 restatement, max over the eight test pages
F16_LOGIT_BOUND = 2 * F16_LOGIT_ERR_MEASURED
MARGIN_FACTOR = 10              # the project's margin rule
SET_ASIDE_CAP = 0.25


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """base config, eight seeded pages, their encoding, the fp32 restatement's hidden states and logits"""
    d = tmp_path_factory.mktemp("bpe")
    write_synthetic_bpe(str(d), seed=1)
    tok = ByteLevelBPE(str(d / "vocab.json"), str(d / "merges.txt"))
    pages = R.make_test_pages(8)
    ids, bbox, mask = R.encode_test_pages(pages, tok)
    state = make_layoutlmv3_state(0)
    pv, resized = R.pixel_values_from_pages([p for p, _, _ in pages])
    with torch.no_grad():
        hid, logits = R.forward(state, R.BASE_CFG, ids, bbox, mask, pv, torch.float32)
    return dict(dir=str(d), pages=pages, ids=ids, bbox=bbox, mask=mask, state=state, resized=resized, hidden=hid.numpy(),
                logits=logits.numpy())


def _model(ctx, case, prec):
    from marie_icr_amd.layoutlmv3 import LayoutLMv3Model, default_config

    return LayoutLMv3Model(ctx, case["state"], default_config(ctx.lib, num_labels=R.BASE_CFG["num_labels"]), prec)


def test_fp32_parity_at_full_size(ctx, case):
    from marie_icr_amd._lib import PREC_F32

    assert case["mask"].sum(1).min() == 2 and case["mask"].sum(1).max() == 512
    m = _model(ctx, case, PREC_F32)
    out = m.forward_host([p for p, _, _ in case["pages"]], case["ids"], case["bbox"], case["mask"], want_hidden=True,
                         want_resized=True)
    m.close()
    assert np.array_equal(out["resized"], case["resized"]), "the resized page differs from Pillow's BILINEAR"
    valid = np.concatenate([case["mask"], np.ones((8, 197), np.int32)], axis=1).astype(bool)
    d_h = float(np.abs(out["hidden"] - case["hidden"])[valid].max())
    d_l = float(np.abs(out["logits"] - case["logits"]).max())
    print(f"fp32: max|d hidden| (valid rows) = {d_h:.3e}, max|d logits| = {d_l:.3e}")
    assert np.isfinite(out["hidden"]).all()
    assert d_h <= FP32_BAR and d_l <= FP32_BAR


def _attention_case(n_tok, masked, seed, heads=2):
    rng = np.random.default_rng(seed)
    D = heads * 64
    q, k, v = (rng.standard_normal((n_tok, D)).astype(np.float32) for _ in range(3))
    n_text = max(n_tok - 197, 0)
    pos = np.concatenate([np.arange(n_text), np.arange(n_tok - n_text)]).astype(np.int32)
    x = rng.integers(0, 1001, n_tok).astype(np.int32)
    y = rng.integers(0, 1001, n_tok).astype(np.int32)
    valid = np.ones(n_tok, np.int32)
    if masked:
        valid[rng.random(n_tok) < 0.4] = 0
        valid[: min(70, n_tok // 3)] = 0          # a whole first key tile masked
        valid[-1] = 1
    w1 = rng.uniform(-4, 4, (heads, 32)).astype(np.float32)
    wx = rng.uniform(-4, 4, (heads, 64)).astype(np.float32)
    wy = rng.uniform(-4, 4, (heads, 64)).astype(np.float32)
    return q, k, v, pos, x, y, valid, w1, wx, wy


def _attention_fp64(q, k, v, pos, x, y, valid, w1, wx, wy, round16):
    """softmax(q k^T / 8 + (B1[b32(pj - pi)] + Bx[b64(xj - xi)] + By[b64(yj - yi)]) / 8 + mask) v in float64; operands rounded
    to f16 as the kernel's are when round16 (q after its 1/8 log2(e) pre-scale, which the kernel applies before rounding)"""
    heads = w1.shape[0]
    tq, tk, tv = (torch.from_numpy(a).double() for a in (q, k, v))
    if round16:
        s = 0.125 * 1.4426950408889634
        tq = (torch.from_numpy(q) * np.float32(s)).half().double() / s
        tk, tv = torch.from_numpy(k).half().double(), torch.from_numpy(v).half().double()
    tp, tx, ty = (torch.from_numpy(a).long() for a in (pos, x, y))
    b1 = R.relative_position_bucket(tp[None, :] - tp[:, None], 32, 128)
    bx = R.relative_position_bucket(tx[None, :] - tx[:, None], 64, 256)
    by = R.relative_position_bucket(ty[None, :] - ty[:, None], 64, 256)
    out = []
    for h in range(heads):
        sl = slice(h * 64, (h + 1) * 64)
        bias = torch.from_numpy(w1[h]).double()[b1] + torch.from_numpy(wx[h]).double()[bx] + torch.from_numpy(wy[h]).double()[by]
        s = tq[:, sl] @ tk[:, sl].T / 8 + bias / 8
        s = s.masked_fill(~torch.from_numpy(valid).bool()[None, :], float("-inf"))
        out.append(torch.softmax(s, dim=-1) @ tv[:, sl])
    return torch.cat(out, dim=1).numpy()


ATTN_CASES = [(197, False), (200, False), (709, False), (197, True), (200, True), (709, True)]


@pytest.mark.parametrize("n_tok,masked", ATTN_CASES)
def test_attention_kernel_fp32_vs_fp64(ctx, n_tok, masked):
    """bound: 1e-5 relative to the largest output (measured on an MI355X: 4.4e-7 .. 6.9e-7 over the six cases)"""
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.layoutlmv3 import attention_bias_host

    args = _attention_case(n_tok, masked, 40 + n_tok)
    got = attention_bias_host(ctx, PREC_F32, *args)
    ref = _attention_fp64(*args, round16=False)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"attention fp32 n={n_tok} masked={masked}: max err / max|out| = {err:.3e} (bound {FP32_ATTN_BAR:.1e})")
    assert err <= FP32_ATTN_BAR


@pytest.mark.parametrize("n_tok,masked", ATTN_CASES)
def test_attention_kernel_f16_vs_fp64(ctx, n_tok, masked):
    from marie_icr_amd._lib import PREC_F16
    from marie_icr_amd.layoutlmv3 import attention_bias_host

    args = _attention_case(n_tok, masked, 40 + n_tok)
    got = attention_bias_host(ctx, PREC_F16, *args)
    ref = _attention_fp64(*args, round16=True)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"attention f16 n={n_tok} masked={masked}: max err / max|out| = {err:.3e} (bound {F16_ATTN_BOUND:.3e})")
    assert np.isfinite(got).all()
    assert err <= F16_ATTN_BOUND


def test_f16_mode_keeps_label_and_score_under_the_margin_rule(ctx, case):
    from marie_icr_amd._lib import PREC_F16

    m = _model(ctx, case, PREC_F16)
    out = m.forward_host([p for p, _, _ in case["pages"]], case["ids"], case["bbox"], case["mask"])
    m.close()
    ref = case["logits"]
    err = np.abs(out["logits"] - ref).max(1)
    print("f16: max|d logits| per page =", err, f"(bound {F16_LOGIT_BOUND:.3e})")
    assert float(err.max()) <= F16_LOGIT_BOUND
    top = np.sort(ref, axis=1)
    kept = (top[:, -1] - top[:, -2]) > MARGIN_FACTOR * F16_LOGIT_ERR_MEASURED
    print("pages kept by the margin rule:", kept)
    assert 1.0 - kept.mean() <= SET_ASIDE_CAP

    def softmax(z):
        e = np.exp(z - z.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)

    p16, p32 = softmax(out["logits"].astype(np.float64)), softmax(ref.astype(np.float64))
    for i in np.nonzero(kept)[0]:
        k = int(ref[i].argmax())
        assert int(out["logits"][i].argmax()) == k, f"page {i}: label differs"
        assert abs(p16[i, k] - p32[i, k]) <= F16_LOGIT_ERR_MEASURED, f"page {i}: score differs"


def test_predict_batch_equals_one_page_calls_bitwise_fp32(ctx, case):
    cfg = dict(R.BASE_CFG, id2label={str(i): f"class_{i}" for i in range(R.BASE_CFG["num_labels"])})
    with open(os.path.join(case["dir"], "config.json"), "w") as f:
        json.dump(cfg, f)
    clf = TransformersDocumentClassifier(case["dir"], state=case["state"], precision="f32", ctx=ctx)
    sizes = [(3300, 2550), (1100, 850), (330, 255)]
    frames, words, boxes = [], [], []
    from marie_icr_amd.renderer import get_words_and_boxes
    from marie_icr_amd.weights import make_ocr_result

    for i in range(16):
        h, w = sizes[i % 3]
        frames.append(make_page_bgr(300 + i, h, w))
        wd, bx = get_words_and_boxes([make_ocr_result(400 + i, w, h, n_lines=(2, 9, 30, 70)[i % 4])], 0)
        words.append(wd)
        boxes.append(bx)
    batch = clf.predict(frames, words, boxes, batch_size=16)
    single = [clf.predict_document_image(f, w, b)[0] for f, w, b in zip(frames, words, boxes)]
    clf.close()
    assert len(batch) == 16
    for i, (b, s) in enumerate(zip(batch, single)):
        assert b["label"] == s["label"] and b["score"] == s["score"], (i, b, s)
        assert b["details"] == {s["label"]: s["score"]}
