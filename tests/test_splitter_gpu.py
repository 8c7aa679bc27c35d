"""GPU parity of the document splitter: the LANCZOS page resize against Pillow byte for byte (the host ABI and the batched
fragment path of a LayoutLMv3 handle), the fp32 model fed the LANCZOS pages against the fp32 torch restatement, the f16 mode
under the margin rule, and ``predict`` in batches against one-page calls."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layoutlmv3_ref as R  # noqa: E402
from test_layoutlmv3_gpu import F16_LOGIT_ERR_MEASURED  # noqa: E402  (the f16 logit error the classifier's tests carry)

from marie_icr_amd.document_classifier import ByteLevelBPE  # noqa: E402
from marie_icr_amd.weights import make_layoutlmv3_state, make_ocr_result, make_page_bgr, write_synthetic_bpe  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_BAR = 1e-3                 # the project's standing fp32 bar on logits
SCORE_BAR = 1e-5                # soft-max score against the restatement's
F16_MARGIN = 2 * F16_LOGIT_ERR_MEASURED      # both of the top two logits may move by the error: a larger gap keeps the label
LAYERS = 2                      # the smallest configuration of the LayoutLMv3 GPU tests: base widths, two layers
CFG = dict(R.BASE_CFG, num_hidden_layers=LAYERS)
# Chosen with the CPU restatement alone (fp32, Pillow-LANCZOS pages), before any GPU run: state seed 0, page seeds 500..503,
# OCR seeds 600..603 (401, 73, 512 and 21 tokens: the third page is truncated).  Top-two logit margins of the four pages:
# 2.306, 8.971, 6.299, 21.187 — all above F16_MARGIN (0.1258), so the margin rule sets no page aside.
STATE_SEED, PAGE_SEED, OCR_SEED = 0, 500, 600
PAGE_SIZES = ((1100, 850), (330, 255))


def _pages(n, page_seed, ocr_seed, lines=(9, 30, 70, 2, 14)):
    """n seeded frames of the two sizes in turn, each with its own OCR words and boxes"""
    from marie_icr_amd.renderer import get_words_and_boxes

    frames, words, boxes = [], [], []
    for i in range(n):
        h, w = PAGE_SIZES[i % 2]
        frames.append(make_page_bgr(page_seed + i, h, w))
        wd, bx = get_words_and_boxes([make_ocr_result(ocr_seed + i, w, h, n_lines=lines[i % len(lines)])], 0)
        words.append(wd)
        boxes.append(bx)
    return frames, words, boxes


def _lanczos(pages, size=224):
    return np.stack([np.asarray(Image.fromarray(p).resize((size, size), Image.LANCZOS)) for p in pages])


def build_case(directory, state_seed=STATE_SEED, page_seed=PAGE_SEED, ocr_seed=OCR_SEED):
    """four pages of two sizes, their encoding, the seeded two-layer state and the fp32 restatement's logits on the
    Pillow-LANCZOS pages (CPU only)"""
    write_synthetic_bpe(directory, seed=1)
    tok = ByteLevelBPE(os.path.join(directory, "vocab.json"), os.path.join(directory, "merges.txt"))
    frames, words, boxes = _pages(4, page_seed, ocr_seed)
    ids, bbox, mask = R.encode_test_pages(list(zip(frames, words, boxes)), tok)
    state = make_layoutlmv3_state(state_seed, layers=LAYERS)
    resized = _lanczos(frames)
    pv = torch.from_numpy((resized.astype(np.float64) / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        logits = R.forward(state, CFG, ids, bbox, mask, pv, torch.float32)[1].numpy()
    return dict(dir=directory, frames=frames, words=words, boxes=boxes, ids=ids, bbox=bbox, mask=mask, state=state,
                resized=resized, logits=logits)


def _softmax(z):
    e = np.exp(z.astype(np.float64) - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _margins(logits):
    top = np.sort(logits, axis=1)
    return top[:, -1] - top[:, -2]


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return build_case(str(tmp_path_factory.mktemp("splitter")))


def _model(ctx, case, prec, resample=None):
    from marie_icr_amd.layoutlmv3 import LayoutLMv3Model, default_config

    m = LayoutLMv3Model(ctx, case["state"], default_config(ctx.lib, layers=LAYERS, num_labels=CFG["num_labels"]), prec)
    if resample is not None:
        m.set_resample(resample)
    return m


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ 1. the host ABI
RESIZE_SHAPES = [((257, 331), (224, 224)),      # a non-integer ratio near 1.3
                 ((540, 700), (224, 224)),      # windows of 8 to 10 taps
                 ((37, 100), (224, 224)),       # an enlargement: the filter scale clamped to 1
                 ((224, 224), (224, 224)),
                 ((50, 1), (224, 224)),         # a one-pixel-wide source: every window clipped at both borders
                 ((330, 255), (64, 48))]        # a non-square target


@pytest.mark.parametrize("src,dst", RESIZE_SHAPES)
def test_lanczos_resize_host_abi_equals_pillow_bytewise(ctx, src, dst):
    from marie_icr_amd.dit import pil_resize_rgb
    from marie_icr_amd.layoutlmv3 import PIL_LANCZOS

    a = _noise(1000 + src[0] + src[1], *src)
    want = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), Image.LANCZOS))
    got = pil_resize_rgb(ctx, a, dst, filter=PIL_LANCZOS)
    diff = got != want
    print(f"LANCZOS {src} -> {dst}: {int(diff.sum())} of {diff.size} bytes differ")
    assert np.array_equal(got, want)


def test_unknown_filters_are_refused(ctx, case):
    from marie_icr_amd._lib import MarieHipError, PREC_F32
    from marie_icr_amd.dit import pil_resize_rgb

    for bad in (0, 4, 5):
        with pytest.raises(MarieHipError):
            pil_resize_rgb(ctx, _noise(1, 20, 30), (8, 8), filter=bad)
    m = _model(ctx, case, PREC_F32)
    for bad in (0, 4, -1):
        with pytest.raises(MarieHipError, match="resample"):
            m.set_resample(bad)
    m.close()


# ------------------------------------------------------------------------------------------------ 2. the fragment path
def test_lanczos_handle_resizes_packed_pages_as_pillow_and_default_stays_bilinear(ctx, case):
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.layoutlmv3 import PIL_LANCZOS

    pages = [_noise(7, 257, 331), _noise(8, 540, 700), _noise(9, 120, 90)]
    ids, bbox, mask = (np.repeat(a[:1], 3, axis=0) for a in (case["ids"], case["bbox"], case["mask"]))
    m = _model(ctx, case, PREC_F32, PIL_LANCZOS)
    got = m.forward_host(pages, ids, bbox, mask, want_resized=True)["resized"]
    m.close()
    want = _lanczos(pages)
    for i in range(3):
        print(f"page {i} {pages[i].shape[:2]}: {int((got[i] != want[i]).sum())} bytes differ from Pillow LANCZOS")
    assert np.array_equal(got, want)
    default = _model(ctx, case, PREC_F32)
    plain = default.forward_host(pages[:1], ids[:1], bbox[:1], mask[:1], want_resized=True)["resized"]
    default.close()
    assert np.array_equal(plain[0], np.asarray(Image.fromarray(pages[0]).resize((224, 224), Image.BILINEAR)))
    assert not np.array_equal(plain[0], got[0])


# ------------------------------------------------------------------------------------------------ 3. fp32 model parity
def test_fp32_logits_equal_the_restatement_on_lanczos_pages(ctx, case):
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.layoutlmv3 import PIL_LANCZOS

    m = _model(ctx, case, PREC_F32, PIL_LANCZOS)
    out = m.forward_host(case["frames"], case["ids"], case["bbox"], case["mask"], want_resized=True)
    m.close()
    assert np.array_equal(out["resized"], case["resized"]), "the resized pages differ from Pillow's LANCZOS"
    ref = case["logits"]
    d_l = float(np.abs(out["logits"] - ref).max())
    d_s = float(np.abs(_softmax(out["logits"]) - _softmax(ref)).max(1).max())
    print(f"fp32 splitter: max|d logits| = {d_l:.3e} (bar {FP32_BAR:.0e}), max|d score| = {d_s:.3e} (bar {SCORE_BAR:.0e}), "
          f"margins = {_margins(ref)}")
    assert np.isfinite(out["logits"]).all() and d_l <= FP32_BAR
    assert np.array_equal(out["logits"].argmax(1), ref.argmax(1))
    k = ref.argmax(1)
    rows = np.arange(len(k))
    assert float(np.abs(_softmax(out["logits"])[rows, k] - _softmax(ref)[rows, k]).max()) <= SCORE_BAR


# ------------------------------------------------------------------------------------------------ 4. f16
def test_f16_keeps_the_labels_under_the_margin_rule(ctx, case):
    """The label is the restatement's wherever its top-two margin exceeds twice the f16 logit error the classifier's tests
    carry; that rule is sound while the f16 logits stay within that error, which is asserted too."""
    from marie_icr_amd._lib import PREC_F16
    from marie_icr_amd.layoutlmv3 import PIL_LANCZOS

    ref = case["logits"]
    kept = _margins(ref) > F16_MARGIN
    assert (~kept).sum() <= 1, f"the seeded pages leave {int((~kept).sum())} pages without a margin: {_margins(ref)}"
    m = _model(ctx, case, PREC_F16, PIL_LANCZOS)
    out = m.forward_host(case["frames"], case["ids"], case["bbox"], case["mask"])
    m.close()
    err = np.abs(out["logits"] - ref).max(1)
    print(f"f16 splitter: max|d logits| per page = {err} (the classifier's constant: {F16_LOGIT_ERR_MEASURED:.3e}), "
          f"margins = {_margins(ref)}, kept = {kept}")
    assert np.isfinite(out["logits"]).all()
    assert float(err.max()) <= F16_LOGIT_ERR_MEASURED
    assert np.array_equal(out["logits"].argmax(1)[kept], ref.argmax(1)[kept])


# ------------------------------------------------------------------------------------------------ 5. batching and pairing
class _Doc:
    def __init__(self, tensor):
        self.tensor, self.tags = tensor, {}


def test_predict_in_batches_equals_one_page_calls_and_pairs_page_i_with_words_i(ctx, case):
    from marie_icr_amd import TransformersDocumentSplitter

    cfg = dict(CFG, id2label={str(i): f"split_{i}" for i in range(CFG["num_labels"])})
    with open(os.path.join(case["dir"], "config.json"), "w") as f:
        json.dump(cfg, f)
    sp = TransformersDocumentSplitter(case["dir"], state=case["state"], precision="f32", ctx=ctx, batch_size=16)
    frames, words, boxes = _pages(5, 700, 800)
    assert len({tuple(w) for w in words}) == 5
    seen, model_call = [], sp._logits
    sp._logits = lambda *a: seen.append(model_call(*a)) or seen[-1]      # the logits behind the scores, call by call
    batch = sp.predict(frames, words, boxes, batch_size=2)
    assert [len(z) for z in seen] == [2, 2, 1]
    single = [sp.predict_document_image(f, w, b) for f, w, b in zip(frames, words, boxes)]
    # what the reference's zip against the whole lists computes for page 2 (the first page's words) is another result
    sp.predict_document_image(frames[2], words[0], boxes[0])
    crossed_gap = float(np.abs(seen[-1][0] - seen[1][0]).max())
    print(f"page 2 with the first page's words: max|d logits| = {crossed_gap:.3e}")
    assert crossed_gap > 100 * FP32_BAR
    docs = [_Doc(f) for f in frames[:3]]
    back = sp.run(docs, words[:3], boxes[:3], batch_size=2)
    none = sp.run([])
    sp.close()
    assert len(batch) == 5 and none == []
    for i, (b, s) in enumerate(zip(batch, single)):
        assert len(s) == 1 and set(s[0]) == {"label", "score"}
        assert b["label"] == s[0]["label"] and abs(b["score"] - s[0]["score"]) <= 1e-6, (i, b, s)
        assert set(b) == {"label", "score", "details"} and b["details"] == {b["label"]: b["score"]}
    assert back is docs
    for d, b in zip(docs, batch):
        t = d.tags["split"]
        assert set(t) == {"label", "score", "details"} and t["details"][t["label"]] == t["score"]
        assert t["label"] == b["label"] and abs(t["score"] - b["score"]) <= 1e-6
        assert "classification" not in d.tags
