"""Restatements for the document boundary registration tests (test infrastructure, not product code).

* ``fast_rcnn_inference_multi`` — detectron2 v0.6 fast_rcnn_inference_single_image for K classes + detector_postprocess,
  with torchvision's GPU batched_nms (<= 20 000 box coordinates: ``_batched_nms_coordinate_trick``) and nms kernel (stable
  descending sort, IoU > threshold in fp32).  Softmax: max and sum left to right, exp(x - max) / sum, exp rounded from double.
* ``resize_area_any`` — cv2.resize(..., INTER_AREA) for 8-bit 3-channel images: a copy for equal sizes, the area shrink of
  oracle/ingest_ref.py when neither axis grows, otherwise OpenCV's generic linear resampler with INTER_AREA's coefficients
  (imgproc resize.cpp: area-mode xofs / ialpha, HResizeLinear, the scalar VResizeLinear with FixedPtCast<int, uchar, 22>).
* ``circle_fill`` — cv2.circle(img, c, r, colour, -1) with LINE_8: drawing.cpp's integer Circle() fill, line by line.
* ``predict_document_image_ref`` — marie/components/document_registration/unilm_dit.py:375-508 restated literally
  (debug_visualization forced on, as the reference's constructor does; no debug writes).

None of these is pinned by a fixture: OpenCV, detectron2 and torchvision are not available to the tests, so they are
restatements of the published algorithms (PARITY UNPINNED, like oracle/ingest_ref.py's resamplers).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import ingest_ref
from oracle.dit_torch import nms as _nms_torch

SCALE_CLAMP = np.float32(math.log(1000.0 / 16))
F32 = np.float32


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a))


def exp_cr(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, np.float64)).astype(np.float32)


def nms_gpu(boxes: np.ndarray, scores: np.ndarray, thr: float) -> np.ndarray:
    """torchvision.ops.nms: stable descending score order, suppress IoU > thr (fp32)"""
    if len(boxes) == 0:
        return np.zeros((0,), np.int64)
    return _nms_torch(_t(boxes.astype(np.float32)), _t(scores.astype(np.float32)), thr).numpy()


def batched_nms(boxes: np.ndarray, scores: np.ndarray, idxs: np.ndarray, thr: float) -> np.ndarray:
    """torchvision.ops.batched_nms, coordinate-offset path"""
    if len(boxes) == 0:
        return np.zeros((0,), np.int64)
    boxes = boxes.astype(np.float32)
    max_coordinate = boxes.max()
    offsets = np.asarray(idxs).astype(np.float32) * (max_coordinate + F32(1))
    return nms_gpu(boxes + offsets[:, None], scores, thr)


def _decode(deltas: np.ndarray, rois: np.ndarray) -> np.ndarray:
    """Box2BoxTransform(10, 10, 5, 5).apply_deltas for one class: deltas (n, 4), rois (n, 4)"""
    with np.errstate(over="ignore", invalid="ignore"):
        widths = rois[:, 2] - rois[:, 0]
        heights = rois[:, 3] - rois[:, 1]
        ctr_x = rois[:, 0] + F32(0.5) * widths
        ctr_y = rois[:, 1] + F32(0.5) * heights
        dx, dy = deltas[:, 0] / F32(10), deltas[:, 1] / F32(10)
        dw, dh = deltas[:, 2] / F32(5), deltas[:, 3] / F32(5)
        dw = np.where(dw > SCALE_CLAMP, SCALE_CLAMP, dw)           # torch.clamp(max=): NaN stays NaN
        dh = np.where(dh > SCALE_CLAMP, SCALE_CLAMP, dh)
        pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
        pw, ph = exp_cr(dw) * widths, exp_cr(dh) * heights
        return np.stack([pcx - F32(0.5) * pw, pcy - F32(0.5) * ph, pcx + F32(0.5) * pw, pcy + F32(0.5) * ph], 1)


def fast_rcnn_inference_multi(head: np.ndarray, rois: np.ndarray, K: int, img_hw, page_hw, score_thr=0.05, nms_thr=0.5,
                              max_det=100):
    """head (n, 5K + 1): K + 1 logits (background last) then 4K class-specific deltas -> (boxes, scores, classes)"""
    head = np.asarray(head, np.float32)
    rois = np.asarray(rois, np.float32)
    n = len(rois)
    logits = head[:, : K + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        mx = logits[:, 0].copy()
        for j in range(1, K + 1):
            mx = np.fmax(mx, logits[:, j])
        e = exp_cr(logits - mx[:, None])
        s = np.zeros((n,), np.float32)
        for j in range(K + 1):
            s = s + e[:, j]
        probs = e / s[:, None]
    boxes = np.stack([_decode(head[:, K + 1 + 4 * j: K + 5 + 4 * j], rois) for j in range(K)], 1)   # (n, K, 4)
    valid = np.isfinite(boxes).all(axis=(1, 2)) & np.isfinite(probs).all(axis=1)
    boxes, probs = boxes[valid], probs[valid]
    scores = probs[:, :K]
    h, w = img_hw
    boxes = boxes.copy()
    boxes[..., 0::2] = np.clip(boxes[..., 0::2], 0, w)
    boxes[..., 1::2] = np.clip(boxes[..., 1::2], 0, h)
    r, c = np.nonzero(scores > F32(score_thr))
    b, sc = boxes[r, c], scores[r, c]
    keep = batched_nms(b, sc, c, nms_thr)[:max_det]
    b, sc, c = b[keep], sc[keep], c[keep]
    sx, sy = np.float32(page_hw[1] / w), np.float32(page_hw[0] / h)
    b = b * np.array([sx, sy, sx, sy], np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, page_hw[1])
    b[:, 1::2] = np.clip(b[:, 1::2], 0, page_hw[0])
    ne = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
    return b[ne], sc[ne], c[ne].astype(np.int32)


# ---------------------------------------------------------------------------------------------------- cv2 pieces
def _linear_area_tab(ssize: int, dsize: int, clamp_last: bool):
    inv = dsize / ssize
    scale = 1.0 / inv
    d = np.arange(dsize)
    s = np.floor(d * scale).astype(np.int64)
    f = ((d + 1) - (s + 1) * inv).astype(np.float32)
    f = np.where(f <= 0, F32(0), f - np.floor(f)).astype(np.float32)
    if clamp_last:
        last = s >= ssize - 1
        f[last] = 0
        s[last] = ssize - 1
    a0 = np.clip(np.rint((F32(1) - f) * F32(2048)), -32768, 32767).astype(np.int64)
    a1 = np.clip(np.rint(f * F32(2048)), -32768, 32767).astype(np.int64)
    return s, a0, a1


def resize_area_linear(img: np.ndarray, new_width: int, new_height: int) -> np.ndarray:
    """cv2.resize INTER_AREA when an axis enlarges (the generic linear resampler, area-mode coefficients), uint8 HxWx3"""
    sh, sw, _ = img.shape
    sx, ax0, ax1 = _linear_area_tab(sw, new_width, True)
    sy, by0, by1 = _linear_area_tab(sh, new_height, False)
    src = img.astype(np.int64)
    one = sx + 1 >= sw
    nxt = np.minimum(sx + 1, sw - 1)
    hor = np.where(one[None, :, None], src[:, sx, :] * 2048,
                   src[:, sx, :] * ax0[None, :, None] + src[:, nxt, :] * ax1[None, :, None])     # (sh, dw, 3)
    y0 = np.clip(sy, 0, sh - 1)
    y1 = np.clip(sy + 1, 0, sh - 1)
    v = (hor[y0] * by0[:, None, None] + hor[y1] * by1[:, None, None] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


def resize_area_any(img: np.ndarray, new_width: int, new_height: int) -> np.ndarray:
    sh, sw = img.shape[:2]
    if new_width <= 0 or new_height <= 0:
        raise ValueError("cv2.resize: empty destination")
    if (new_width, new_height) == (sw, sh):
        return img.copy()
    if new_width <= sw and new_height <= sh:
        return ingest_ref.resize_area(img, new_width, new_height)
    return resize_area_linear(img, new_width, new_height)


def circle_fill(img: np.ndarray, center, radius: int, color) -> None:
    """drawing.cpp Circle(img, center, radius, color, fill=1), in place"""
    H, W = img.shape[:2]
    cx, cy = center
    color = np.asarray(color, np.uint8)
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    inside = cx >= radius and cx < W - radius and cy >= radius and cy < H - radius

    def hline(y, xl, xr):
        img[y, xl:xr + 1] = color

    while dx >= dy:
        y11, y12, y21, y22 = cy - dy, cy + dy, cy - dx, cy + dx
        x11, x12, x21, x22 = cx - dx, cx + dx, cx - dy, cx + dy
        if inside:
            hline(y11, x11, x12)
            hline(y12, x11, x12)
            hline(y21, x21, x22)
            hline(y22, x21, x22)
        elif x11 < W and x12 >= 0 and y21 < H and y22 >= 0:
            x11, x12 = max(x11, 0), min(x12, W - 1)
            if 0 <= y11 < H:
                hline(y11, x11, x12)
            if 0 <= y12 < H:
                hline(y12, x11, x12)
            if x21 < W and x22 >= 0:
                x21, x22 = max(x21, 0), min(x22, W - 1)
                if 0 <= y21 < H:
                    hline(y21, x21, x22)
                if 0 <= y22 < H:
                    hline(y22, x21, x22)
        dy += 1
        err += plus
        plus += 2
        mask = (err <= 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2


def copy_make_border(img, top, bottom, left, right, value=(255, 255, 255)):
    out = np.empty((img.shape[0] + top + bottom, img.shape[1] + left + right, 3), np.uint8)
    out[...] = np.asarray(value, np.uint8)
    out[top:top + img.shape[0], left:left + img.shape[1]] = img
    return out


# ---------------------------------------------------------------------------------------------------- unilm_dit.py
def predict_document_image_ref(image, boxes, scores, classes, registration_mode, registration_point=(10, 10),
                               margin_width=5, margin_height=5, images=True):
    """unilm_dit.py:375-508 on the detector's (boxes, scores, classes).  Returns a dict of the prediction's fields plus a
    trace of the intermediate shapes; ``images=False`` skips the pixel work (shapes only)."""
    width, height = image.shape[1], image.shape[0]
    default = {"detected": False, "boundary_bbox": [0, 0, 0, 0], "score": 0, "aligned_image": None, "trace": None}
    boxes, scores, classes = np.asarray(boxes, np.float32), np.asarray(scores, np.float32), np.asarray(classes)
    if len(boxes) == 0:
        return default
    if len(boxes) > 1:
        min_score = 0.7
        indices = np.where(scores > min_score)
        scores, boxes, classes = scores[indices], boxes[indices], classes[indices]
        if len(boxes) == 0:
            return default
        keep = batched_nms(boxes.astype(np.float32), scores.astype(np.float32), classes, 0.5)
        keep = keep[:1]
        boxes, scores, classes = [boxes[keep[0]]], [scores[keep[0]]], [classes[keep[0]]]
    boundary_bbox = [int(x) for x in boxes[0]]
    x0, y0, x1, y1 = boundary_bbox
    w, h = x1 - x0, y1 - y0
    x, y = x0, y0
    p1_x, p1_y = registration_point
    boundary_bbox = [max(0, x - margin_width), max(0, y - margin_height), min(width, w + margin_width * 2),
                     min(height, h + margin_height * 2)]
    score = scores[0]
    aligned_image = np.ones((height, width, 3), dtype=np.uint8) * 255
    boundary = image[boundary_bbox[1]: boundary_bbox[1] + boundary_bbox[3],
                     boundary_bbox[0]: boundary_bbox[0] + boundary_bbox[2]]
    trace = {"crop_shape": boundary.shape[:2], "resized_shape": None, "border": None, "markers": []}
    if registration_mode == "absolute":
        if p1_x + boundary_bbox[2] > width:
            return default
        if p1_y + boundary_bbox[3] > height:
            return default
        aligned_image[p1_y: p1_y + boundary.shape[0], p1_x: p1_x + boundary.shape[1]] = boundary
        trace["resized_shape"] = boundary.shape[:2]
        trace["border"] = (p1_y, p1_x)
        trace["markers"] = [(p1_x, p1_y)]
        if images:
            circle_fill(aligned_image, (p1_x, p1_y), 8, (0, 0, 255))
    elif registration_mode == "fit_to_page":
        new_width = width - p1_x * 2
        resized_shape = boundary.shape[:2]
        resized_boundary = boundary
        if boundary_bbox[3] > boundary_bbox[2]:
            (bh_, bw_) = boundary.shape[:2]
            r = new_width / float(bw_)
            dim = (new_width, int(bh_ * r))
            resized_shape = (dim[1], dim[0])
            if images:
                resized_boundary = resize_area_any(boundary, dim[0], dim[1])
        boundary_height, boundary_width = resized_shape
        bottom = height - boundary_height - p1_y
        bottom = max(0, int(bottom))
        trace["resized_shape"] = resized_shape
        trace["border"] = (p1_y, bottom, p1_x, p1_x)
        trace["markers"] = [(p1_x, p1_y), (p1_x + new_width, p1_y)]
        aligned_shape = (boundary_height + p1_y + bottom, boundary_width + 2 * p1_x)
        if images:
            aligned_image = copy_make_border(resized_boundary, p1_y, bottom, p1_x, p1_x)
            circle_fill(aligned_image, (p1_x, p1_y), 8, (0, 0, 255))
            circle_fill(aligned_image, (p1_x + new_width, p1_y), 8, (0, 0, 255))
        else:
            aligned_image = np.empty(aligned_shape + (3,), np.uint8)
    trace["aligned_shape"] = aligned_image.shape[:2]
    if aligned_image.shape[0] != image.shape[0] or aligned_image.shape[1] != image.shape[1]:
        if images:
            aligned_image = ingest_ref.resize_cubic(aligned_image, image.shape[1], image.shape[0])
    return {"detected": True, "boundary_bbox": boundary_bbox, "score": float(score),
            "aligned_image": aligned_image if images else None, "trace": trace}
