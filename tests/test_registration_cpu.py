"""Document boundary registration without a GPU: the registration plan (box choice, boundary box, crop, resize, border,
markers, canvas) against the literal restatement of unilm_dit.py:375-508 (tests/registration_ref.py), the prediction
model, the no-op processor and the constructor's errors."""
import numpy as np
import pytest

from registration_ref import predict_document_image_ref

W, H = 300, 400


def _boxes(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 4)


def _scores(*vals):
    return np.asarray(vals, np.float32)


# (name, page (w, h), boxes, scores, mode, registration point)
CASES = [
    ("none", (W, H), _boxes(), _scores(), "absolute", (10, 10)),
    ("one_low_score", (W, H), _boxes([40.7, 50.2, 120.9, 160.5]), _scores(0.06), "absolute", (10, 10)),
    ("many", (W, H), _boxes([40.7, 50.2, 120.9, 160.5], [30, 40, 200, 300], [41, 51, 121, 161]), _scores(0.93, 0.81, 0.2),
     "absolute", (10, 10)),
    ("many_below", (W, H), _boxes([40, 50, 120, 160], [30, 40, 200, 300]), _scores(0.69, 0.5), "absolute", (10, 10)),
    ("top_at_0.7", (W, H), _boxes([40, 50, 120, 160], [30, 40, 200, 300]), _scores(0.7, 0.5), "fit_to_page", (10, 10)),
    ("margins_clipped_absolute", (W, H), _boxes([2.5, 3.9, 298.2, 397.7]), _scores(0.9), "absolute", (0, 0)),
    ("margins_clipped_fit", (W, H), _boxes([2.5, 3.9, 298.2, 397.7]), _scores(0.9), "fit_to_page", (10, 10)),
    ("crop_smaller_than_bbox", (W, H), _boxes([260.3, 330.8, 299.9, 399.2]), _scores(0.9), "absolute", (10, 10)),
    ("absolute_oob_x", (W, H), _boxes([5, 5, 295, 100]), _scores(0.9), "absolute", (10, 10)),
    ("absolute_oob_y", (W, H), _boxes([5, 5, 100, 395]), _scores(0.9), "absolute", (10, 10)),
    ("fit_portrait_shrink", (W, H), _boxes([12.2, 8.1, 288.7, 390.3]), _scores(0.9), "fit_to_page", (10, 10)),
    ("fit_portrait_enlarge", (W, H), _boxes([100.4, 100.6, 150.2, 250.9]), _scores(0.9), "fit_to_page", (10, 10)),
    ("fit_r_equals_1", (W, H), _boxes([15.1, 20.0, 285.9, 390.0]), _scores(0.9), "fit_to_page", (10, 10)),
    ("fit_landscape", (W, H), _boxes([20.5, 50.5, 280.5, 200.5]), _scores(0.9), "fit_to_page", (10, 10)),
    ("fit_integral_shrink", (400, 900), _boxes([5, 5, 395, 805]), _scores(0.9), "fit_to_page", (100, 10)),
    ("unknown_mode", (W, H), _boxes([40.7, 50.2, 120.9, 160.5]), _scores(0.95), "warp_drive", (10, 10)),
]


def _case_ids():
    return [c[0] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=_case_ids())
def test_plan_matches_literal_restatement(case):
    from marie_icr_amd.document_registration import registration_plan

    _, (pw, ph), boxes, scores, mode, point = case
    page = np.zeros((ph, pw, 3), np.uint8)
    ref = predict_document_image_ref(page, boxes, scores, np.zeros(len(boxes), np.int64), mode, point, 5, 5, images=False)
    plan = registration_plan(pw, ph, boxes, scores, mode, point, 5, 5)
    assert plan.detected == ref["detected"]
    if not ref["detected"]:
        return
    assert plan.boundary_bbox == ref["boundary_bbox"]
    assert plan.score == ref["score"]
    assert plan.final == (pw, ph)
    tr = ref["trace"]
    assert (plan.canvas[1], plan.canvas[0]) == tr["aligned_shape"]
    if mode not in ("absolute", "fit_to_page"):
        assert plan.crop[2:] == (0, 0) and plan.markers == []
        return
    assert (plan.crop[3], plan.crop[2]) == tr["crop_shape"]
    assert (plan.resized[1], plan.resized[0]) == tuple(tr["resized_shape"])
    assert plan.offset == (point[0], point[1])
    assert plan.markers == tr["markers"]
    if mode == "fit_to_page":
        top, bottom, left, right = tr["border"]
        assert plan.canvas == (plan.resized[0] + left + right, plan.resized[1] + top + bottom)


def test_case_table_covers_the_paths():
    """the table reaches every branch the issue lists"""
    from marie_icr_amd.document_registration import registration_plan

    plans = {name: registration_plan(pw, ph, b, s, m, pt) for name, (pw, ph), b, s, m, pt in CASES}
    assert not plans["none"].detected and plans["one_low_score"].detected and plans["many"].detected
    assert not plans["many_below"].detected and not plans["top_at_0.7"].detected
    assert not plans["absolute_oob_x"].detected and not plans["absolute_oob_y"].detected
    p = plans["crop_smaller_than_bbox"]
    assert p.crop[2] < p.boundary_bbox[2] and p.crop[3] < p.boundary_bbox[3]
    p = plans["margins_clipped_absolute"]
    assert p.boundary_bbox == [0, 0, W, H]
    p = plans["fit_portrait_shrink"]
    assert p.resized[0] < p.crop[2] and p.resized[1] < p.crop[3]
    p = plans["fit_portrait_enlarge"]
    assert p.resized[0] > p.crop[2] and p.resized[1] > p.crop[3] and p.canvas != p.final
    p = plans["fit_r_equals_1"]
    assert p.resized == p.crop[2:] and p.canvas == p.final
    p = plans["fit_landscape"]
    assert p.resized == p.crop[2:] and p.markers[1][0] >= p.canvas[0] - 8      # second marker clipped by the right border
    p = plans["fit_integral_shrink"]
    assert p.crop[2] == 2 * p.resized[0] and p.crop[3] == 2 * p.resized[1]
    assert plans["unknown_mode"].detected


def test_select_box_equals_the_second_nms():
    """boxes[0] if n == 1 or scores[0] > 0.7 — against the filter + batched_nms + keep[:1] of the reference on random sets"""
    from marie_icr_amd.document_registration import select_box

    rng = np.random.default_rng(7)
    for _ in range(300):
        n = int(rng.integers(0, 8))
        x0, y0 = rng.uniform(0, 200, n), rng.uniform(0, 300, n)
        boxes = np.stack([x0, y0, x0 + rng.uniform(1, 90, n), y0 + rng.uniform(1, 90, n)], 1).astype(np.float32)
        scores = np.sort(rng.choice(np.float32([0.05, 0.3, 0.69, 0.7, 0.71, 0.9, 0.9]), n))[::-1].astype(np.float32)
        classes = rng.integers(0, 5, n)
        ref = predict_document_image_ref(np.zeros((400, 300, 3), np.uint8), boxes, scores, classes, "other", images=False)
        i = select_box(scores)
        assert (i is not None) == ref["detected"]
        if i is not None:
            x0, y0, x1, y1 = (int(v) for v in boxes[i])
            assert ref["boundary_bbox"] == [max(0, x0 - 5), max(0, y0 - 5), min(300, x1 - x0 + 10), min(400, y1 - y0 + 10)]
            assert float(scores[i]) == ref["score"]


def test_prediction_to_dict_and_noop():
    from marie_icr_amd.document_registration import DocumentBoundaryPrediction, NoopDocumentBoundaryRegistration

    img = np.zeros((2, 3, 3), np.uint8)
    p = DocumentBoundaryPrediction(label="document", detected=True, mode="absolute", aligned_image=img,
                                   boundary_bbox=[1, 2, 3, 4], score=0.5)
    assert p.to_dict() == {"label": "document", "detected": True, "mode": "absolute", "boundary_bbox": [1, 2, 3, 4],
                           "score": 0.5}
    d = p.to_dict(include_images=True)
    assert d["aligned_image"] == img.tolist() and d["visualization_image"] is None
    assert list(d) == ["label", "detected", "mode", "aligned_image", "visualization_image", "boundary_bbox", "score"]

    class Doc:
        def __init__(self, t):
            self.tensor, self.tags = t, {}

    docs = [Doc(img), Doc(img)]
    out = NoopDocumentBoundaryRegistration().run(docs, "fit_to_page")
    assert out is docs
    for d in docs:
        b = d.tags["document_boundary"]
        assert (b.detected, b.mode, b.boundary_bbox, b.score, b.aligned_image) == (False, "fit_to_page", [0, 0, 0, 0], 0, None)
    preds = NoopDocumentBoundaryRegistration().run([img])
    assert len(preds) == 1 and not preds[0].detected and preds[0].mode == "absolute"
    with pytest.raises(ValueError):
        NoopDocumentBoundaryRegistration().run([img], "warp_drive")
    with pytest.raises(ValueError):
        NoopDocumentBoundaryRegistration().run([img], "absolute", [10, 10])


def test_missing_checkpoint_and_cpu_requests(tmp_path):
    from marie_icr_amd._lib import MarieHipError
    from marie_icr_amd.document_registration import UnilmDocumentBoundaryRegistration

    with pytest.raises(FileNotFoundError):
        UnilmDocumentBoundaryRegistration("document_boundary", models_dir=str(tmp_path))
    with pytest.raises(MarieHipError):
        UnilmDocumentBoundaryRegistration("document_boundary", use_gpu=False)


def test_boundary_state_and_config():
    from marie_icr_amd.weights import make_dit_boundary_state, make_dit_state

    st, base = make_dit_boundary_state(0), make_dit_state(0)
    p = "roi_heads.box_predictor."
    assert st[p + "cls_score.weight"].shape == (6, 1024) and st[p + "bbox_pred.weight"].shape == (20, 1024)
    assert st[p + "cls_score.bias"].shape == (6,) and st[p + "bbox_pred.bias"].shape == (20,)
    for k, v in base.items():
        if not k.startswith(p):
            assert np.array_equal(st[k], v)


def test_boundary_config():
    from marie_icr_amd import _lib
    from marie_icr_amd.dit import boundary_config, default_config

    import __graft_entry__ as g

    g.build()
    lib = _lib.load()
    assert default_config(lib).num_classes == 1
    c = boundary_config(lib)
    assert (c.model, c.min_size_test, c.max_size_test, c.detections_per_image, c.num_classes) == (0, 800, 1000, 100, 5)
    assert list(c.anchor_sizes) == [32, 64, 128, 256, 512] and list(c.aspect_ratios) == [0.5, 1.0, 2.0]
    assert (c.rpn_nms_thresh, round(c.score_thresh, 6), c.nms_thresh) == (np.float32(0.7), 0.05, 0.5)
