"""Document boundary registration on the GPU: the K-class final stage of the detector, the seeded 5-class detector stage by
stage, the registration warp and ``UnilmDocumentBoundaryRegistration.run`` end to end, each against the restatements of
tests/registration_ref.py (detectron2 / torchvision / OpenCV are not vendored by the reference: parity-unpinned) and the
oracle pieces of oracle/dit_torch.py."""
import numpy as np
import pytest

import registration_ref as ref
from test_registration_cpu import CASES

pytestmark = pytest.mark.gpu

K = 5


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def state():
    from marie_icr_amd.weights import make_dit_boundary_state

    return make_dit_boundary_state(0)


def _equal(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape, (g.shape, w.shape)
        np.testing.assert_array_equal(g, w)


def test_det_final_multi_stage(ctx):
    from marie_icr_amd.dit import det_final_multi

    rng = np.random.default_rng(5)
    n = 1000
    x0, y0 = rng.uniform(0, 700, n), rng.uniform(0, 950, n)
    rois = np.stack([x0, y0, x0 + rng.uniform(4, 300, n), y0 + rng.uniform(4, 400, n)], 1).astype(np.float32)
    rois[300:600] = rois[:300] + rng.normal(0, 2.0, (300, 4)).astype(np.float32)       # near-duplicates: NMS has work
    head = np.concatenate([rng.normal(0, 2, (n, K + 1)), rng.normal(0, 0.5, (n, 4 * K))], 1).astype(np.float32)
    head[:400, K + 5:K + 9] = head[:400, K + 1:K + 5]                 # class 1 boxes = class 0 boxes: no cross-class suppression
    head[700:750], rois[700:750] = head[650:700], rois[650:700]       # identical rows: tied scores, identical boxes
    head[800:850, 1] = head[800:850, 0]                               # tied classes within a row
    head[900:905, 2] = np.nan                                         # non-finite logits / deltas / boxes drop the row
    head[905:910, K + 1 + 7] = np.nan
    head[910, 0] = np.inf
    head[911:915, K + 1 + 2] = np.inf
    head[920:930, K + 1 + 2] = 50.0                                   # the scale clamp
    for max_det in (100, 1000):
        want = ref.fast_rcnn_inference_multi(head, rois, K, (1000, 773), (3300, 2550), max_det=max_det)
        got = det_final_multi(ctx, head, rois, K, (1000, 773), (3300, 2550), max_det=max_det)
        _equal(got, want)
        assert len(set(want[2].tolist())) == K and (max_det != 100 or len(want[0]) == 100)
    assert len(want[0]) > 300
    got = det_final_multi(ctx, head[:0], rois[:0], K, (1000, 773), (3300, 2550))
    assert all(len(g) == 0 for g in got)


def _oracle_stages(state, page):
    from marie_icr_amd.dit import BOUNDARY_ANCHOR_SIZES, BOUNDARY_ASPECT_RATIOS
    from oracle import dit_torch as dt

    o = dt.TorchDitOracle(state, min_size=800, max_size=1000)
    x, hw = o.preprocess(page)
    feats = o.fpn(x)
    cells = dt.cell_anchors(BOUNDARY_ANCHOR_SIZES, BOUNDARY_ASPECT_RATIOS)
    return o, feats, hw, cells


@pytest.mark.parametrize("hw", [(3300, 2550), (255, 330)], ids=["2550x3300", "330x255"])
def test_boundary_detector_stages_fp32(ctx, state, hw):
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.dit import DitModel, boundary_config
    from marie_icr_amd.weights import make_image_u8
    from oracle import dit_torch as dt

    page = make_image_u8(13, 1, hw[0], hw[1])[0]
    m = DitModel(ctx, state, precision=PREC_F32, config=boundary_config(ctx.lib))
    out = m.debug_host(page)
    o, feats, (nh, nw), cells = _oracle_stages(state, page)
    if hw == (3300, 2550):
        assert (nh, nw) == (1000, 773) and m.resized_shape(*hw)[2:] == (1024, 800)
    assert out["resized_hw"] == (nh, nw)
    for l, (f, r) in enumerate(zip(out["fpn"], feats)):
        r = r[0].permute(1, 2, 0).numpy()
        assert f.shape == r.shape and np.abs(f - r).max() <= 2e-3, (l, np.abs(f - r).max())
    # the discrete stages replayed on this run's own tensors give this run's results
    ob, os_ = dt.rpn_proposals(out["rpn_heads"], out["sizes"], (4, 8, 16, 32, 64), (nh, nw), cells)
    assert len(ob) == len(out["proposals"]) and np.abs(ob - out["proposals"]).max() <= 1e-3
    np.testing.assert_array_equal(os_, out["proposal_scores"])
    assert out["head"].shape == (len(out["proposals"]), 5 * K + 1)
    rb, rs, rc = ref.fast_rcnn_inference_multi(out["head"], out["proposals"], K, (nh, nw), page.shape[:2], max_det=100)
    _equal((out["boxes"], out["scores"]), (rb, rs))
    eb, es, ec = m.detect_ex_host(page)[0]
    _equal((eb, es, ec), (rb, rs, rc))
    assert len(rb) == 100
    m.close()


def _page(seed, h, w):
    rng = np.random.default_rng(seed)
    page = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    page[h // 4: h // 2, w // 5: w // 2] = (20, 40, 60)                 # a flat region next to the noise
    return page


EXTRA = [
    ("absolute_marker_right_edge", (300, 400), np.float32([[100.2, 100.0, 100.9, 120.0]]), np.float32([0.9]), "absolute",
     (290, 10)),
    ("fit_marker_bottom_left", (300, 400), np.float32([[20.0, 30.0, 90.0, 390.0]]), np.float32([0.9]), "fit_to_page",
     (5, 396)),
]


@pytest.mark.parametrize("case", CASES + EXTRA, ids=[c[0] for c in CASES + EXTRA])
def test_warp_matches_restatement(ctx, case):
    from marie_icr_amd.document_registration import register_warp_host, registration_plan

    name, (pw, ph), boxes, scores, mode, point = case
    page = _page(len(name), ph, pw)
    plan = registration_plan(pw, ph, boxes, scores, mode, point, 5, 5)
    want = ref.predict_document_image_ref(page, boxes, scores, np.zeros(len(boxes), np.int64), mode, point, 5, 5)
    assert plan.detected == want["detected"]
    if not plan.detected:
        return
    got = register_warp_host(ctx, page, plan)
    assert got.shape == want["aligned_image"].shape
    np.testing.assert_array_equal(got, want["aligned_image"])


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_run_end_to_end(ctx, state, precision):
    from marie_icr_amd.document_registration import UnilmDocumentBoundaryRegistration
    from marie_icr_amd.weights import make_page_bgr

    reg = UnilmDocumentBoundaryRegistration("document_boundary", state=state, precision=precision, ctx=ctx, batch_size=3)
    pages = [make_page_bgr(5 + i, 660, 510) for i in range(4)] + [make_page_bgr(9, 400, 560)]

    class Doc:
        def __init__(self, t):
            self.tensor, self.tags = t, {}

    dets = [reg.model.detect_ex_host(p)[0] for p in pages]
    n_detected = 0
    for mode in ("absolute", "fit_to_page"):
        docs = reg.run([Doc(p) for p in pages], mode)
        for d, page, (b, s, c) in zip(docs, pages, dets):
            got = d.tags["document_boundary"]
            want = ref.predict_document_image_ref(page, b, s, c, mode)
            assert (got.detected, got.boundary_bbox, got.score, got.mode) == (want["detected"], want["boundary_bbox"],
                                                                              want["score"], mode)
            assert got.visualization_image is None
            if want["detected"]:
                n_detected += 1
                np.testing.assert_array_equal(got.aligned_image, want["aligned_image"])
            else:
                assert got.aligned_image is None
    assert n_detected >= 4
    preds = reg.run(pages[:2], "fit_to_page", (20, 30), 7, 3)
    assert len(preds) == 2
    for page, p, (b, s, c) in zip(pages, preds, dets):
        want = ref.predict_document_image_ref(page, b, s, c, "fit_to_page", (20, 30), 7, 3)
        assert p.detected == want["detected"]
        if p.detected:
            np.testing.assert_array_equal(p.aligned_image, want["aligned_image"])
    one = reg.predict_document_image(pages[0], "absolute", (10, 10), 5, 5)
    assert len(one) == 1 and one[0].boundary_bbox == docs[0].tags["document_boundary"].boundary_bbox
    if precision == "f32":
        # against the oracle detector where the choice is not a near-tie: the page's top score clears 0.7 and its runner-up
        # by more than the measured fp32 error, so both sides pick the same box
        from oracle import dit_torch as dt

        page = pages[0]
        o, feats, (nh, nw), cells = _oracle_stages(state, page)
        heads = o.rpn_heads(feats)
        props, _ = dt.rpn_proposals(heads, [tuple(f.shape[2:]) for f in feats], (4, 8, 16, 32, 64), (nh, nw), cells)
        pooled = dt.roi_align([f[0].permute(1, 2, 0).contiguous().numpy() for f in feats[:4]], (1 / 4, 1 / 8, 1 / 16, 1 / 32),
                              props)
        ob, os_, oc = ref.fast_rcnn_inference_multi(o.box_head(pooled), props, K, (nh, nw), page.shape[:2])
        gb, gs, gc = dets[0]
        eps = 2e-3
        if len(os_) > 1 and abs(float(os_[0]) - 0.7) > eps and float(os_[0] - os_[1]) > eps:
            assert (gs[0] > 0.7) == (os_[0] > 0.7) and gc[0] == oc[0]
            assert np.abs(gb[0] - ob[0]).max() <= 1e-2
    reg.close()
