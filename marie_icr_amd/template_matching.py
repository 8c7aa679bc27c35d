"""Template matching on the MI355X: ``VQNNFTemplateMatcher`` (arXiv 2306.15010) and ``MetaTemplateMatcher`` (a template's text
among the OCR words of a page) behind the reference's matcher surface.

Mirrors marie/components/template_matching/{model,base,vqnnf_template_matching,meta_template_matching,
composite_template_maching}.py and the matching core under vqnnf/matching/.

``VQNNFTemplateMatcher``: the reference slices a page into windows and loops in Python over (slice, template),
materialising 128 x H x W fp32 one-hots and integral images for each.  Here the page is uploaded once, the slices are windows
of it, and the nearest-code assignment, the Gauss-Haar heat map and the peak rounds run over the whole (slice x template)
grid in a handful of launches (csrc/vqnnf.hip); only the peaks come back.  Template-side state (k-means codebook, labels,
filter responses) is built once per template and cached under the reference's key ``key_{x}_{y}_{w}_{h}``.

Built: the model-free ``num_features == 27`` colour features of ``PixelFeatureExtractor`` (the paper's colour variant).
The snippet embedding of ``score`` is CLIP's: ``embeddings_processor`` takes an ``OpenAIEmbeddings`` /
``OpenAITransformerEmbeddings`` of ``embeddings.py`` (the ViT towers in HIP) or an ``OpenAIResNetEmbeddings`` (the ModifiedResNet
towers: RN50x4, the reference's default snippet model); the unique clips of a scoring batch go through the encoder in one call.
Or any callable clip -> vector; with None the embedding similarity is taken equal to the feature similarity.
Not built: the EfficientNet hyper-column features and ``pca_lowrank`` (``n_feature != 27`` / ``pca_dims`` raise),
``resize_image_progressive``
(``downscale_factor != 1`` raises), ``DeepDimTemplateMatcher``, and the reference's /tmp/dim writes,
prints and visualisations.  ``slice_image`` and
``GreedyNMMPostprocess`` restate sahi's, which is not installed here: their parity with sahi is not pinned by a golden.

``MetaTemplateMatcher`` slides n-grams of g - 1, g and g + 1 words (g: the words of the template text) over the page's words and
scores each by Levenshtein similarity; n-grams at 0.5 or more also take the cosine of two text embeddings and of two snippet
embeddings, and the three are averaged.  The reference scores one pair at a time in Python; here the page is laid out once as
one string of alphabet ids (``text_layout``), the edit distance of every (template, n-gram) pair comes from one call of
``csrc/lev_ngrams.hip``, and what passes the 0.5 filter goes through the device resize, ``embed_clips`` / ``embed_texts`` and
``pair_cosines`` in batches.  Text embeddings are those of ``text_embeddings_processor`` — ``JinaEmbeddings`` (the reference's
jina-embeddings-v2-base-en) or ``SentenceTransformerEmbeddings`` of embeddings.py, or a callable — or, without one, the CLIP
text tower's.  The distance is the unit-cost edit distance over
code points, exact against the textbook DP; its parity with the ``Levenshtein`` package is not pinned.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import Context, MarieHipError, VqFilters, check
from .dit_box_processor import resize_image
from .ocr_processor import merge_bboxes_as_block
from .renderer import get_words_and_boxes

logger = logging.getLogger(__name__)

N_FEATURES = 27
N_CODE = 128
MAX_FILTERS = 6
CLIP_SIZE = (224, 224)


@dataclass
class TemplateMatchResult:
    """marie/components/template_matching/model.py"""
    bbox: Any
    label: str
    score: float
    similarity: float
    frame_index: Optional[int] = 0


# ---------------------------------------------------------------------------------------------------- slicing and NMM
def slice_image(image_height: int, image_width: int, slice_height: int, slice_width: int,
                overlap_height_ratio: float = 0.2, overlap_width_ratio: float = 0.2) -> List[Tuple[int, int, int, int]]:
    """The windows of sahi.slicing.slice_image(auto_slice_resolution=False) as (x, y, w, h): a step of the slice less an
    overlap of int(ratio * size) pixels; a slice that would overrun the page is moved back inside it."""
    y_overlap, x_overlap = int(overlap_height_ratio * slice_height), int(overlap_width_ratio * slice_width)
    if slice_height <= y_overlap or slice_width <= x_overlap:
        raise ValueError("the overlap must be smaller than the slice")
    out = []
    y_max = y_min = 0
    while y_max < image_height:
        x_min = x_max = 0
        y_max = y_min + slice_height
        while x_max < image_width:
            x_max = x_min + slice_width
            if y_max > image_height or x_max > image_width:
                xm, ym = min(image_width, x_max), min(image_height, y_max)
                x0, y0 = max(0, xm - slice_width), max(0, ym - slice_height)
                out.append((x0, y0, xm - x0, ym - y0))
            else:
                out.append((x_min, y_min, slice_width, slice_height))
            x_min = x_max - x_overlap
        y_min = y_max - y_overlap
    return out


@dataclass
class ObjectPrediction:
    """what GreedyNMMPostprocess works on: an xyxy box, a score and a category"""
    bbox: List[int]
    score: float
    category: str

    def to_xywh(self):
        return [self.bbox[0], self.bbox[1], self.bbox[2] - self.bbox[0], self.bbox[3] - self.bbox[1]]


def box_ios(a: Sequence[float], b: Sequence[float]) -> float:
    """intersection over the smaller area (xyxy)"""
    iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
    inter = max(iw, 0) * max(ih, 0)
    smaller = min((a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1]))
    return inter / smaller if smaller > 0 else 0.0


def box_iou(a: Sequence[float], b: Sequence[float]) -> float:
    iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
    inter = max(iw, 0) * max(ih, 0)
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / union if union > 0 else 0.0


class GreedyNMMPostprocess:
    """Greedy non-maximum merging: per category (unless class_agnostic), highest score first, a kept prediction absorbs
    every remaining one whose match metric with it exceeds ``match_threshold``; a merged pair takes the union box, the
    higher score and that one's category."""

    def __init__(self, match_threshold: float = 0.5, match_metric: str = "IOS", class_agnostic: bool = False):
        if match_metric not in ("IOS", "IOU"):
            raise ValueError(f"match_metric should be IOS or IOU, got {match_metric}")
        self.match_threshold, self.match_metric, self.class_agnostic = match_threshold, match_metric, class_agnostic

    def _metric(self, a, b) -> float:
        return box_ios(a, b) if self.match_metric == "IOS" else box_iou(a, b)

    def __call__(self, predictions: List[ObjectPrediction]) -> List[ObjectPrediction]:
        groups = {}
        for i, p in enumerate(predictions):
            groups.setdefault(None if self.class_agnostic else p.category, []).append(i)
        out = []
        for members in groups.values():
            order = sorted(members, key=lambda i: predictions[i].score, reverse=True)     # stable: ties keep input order
            while order:
                keep, rest = order[0], order[1:]
                matched = [i for i in rest if self._metric(predictions[keep].bbox, predictions[i].bbox) >= self.match_threshold]
                order = [i for i in rest if i not in matched]
                cur = predictions[keep]
                for i in matched:
                    other = predictions[i]
                    if self._metric(cur.bbox, other.bbox) > self.match_threshold:
                        best = cur if cur.score >= other.score else other
                        cur = ObjectPrediction([min(cur.bbox[0], other.bbox[0]), min(cur.bbox[1], other.bbox[1]),
                                                max(cur.bbox[2], other.bbox[2]), max(cur.bbox[3], other.bbox[3])],
                                               best.score, best.category)
                out.append(cur)
        return out


# ---------------------------------------------------------------------------------------------------- base
class BaseTemplateMatcher(ABC):
    """marie/components/template_matching/base.py"""

    DEFAULT_OVERLAP_HEIGHT_RATIO = 0.2
    DEFAULT_OVERLAP_WIDTH_RATIO = 0.2

    def __init__(self, slicing_enabled: bool = True, **kwargs) -> None:
        self.slicing_enabled = slicing_enabled

    @abstractmethod
    def predict(self, frame: np.ndarray, template_frames: List[np.ndarray], template_boxes: List[Sequence[int]],
                template_labels: List[str], template_texts: Optional[List[str]] = None, score_threshold: float = 0.9,
                scoring_strategy: str = "weighted", max_objects: int = 1, batch_size: int = 1, words=None, word_boxes=None,
                word_lines=None) -> List[TemplateMatchResult]:
        """Every location of every template in ``frame`` above the threshold, not filtered for overlap."""

    def predict_windows(self, frame: np.ndarray, windows: List[Tuple[int, int, int, int]], template_frames, template_boxes,
                        template_labels, template_texts, score_threshold, scoring_strategy, max_objects, words=None,
                        word_boxes=None, word_lines=None) -> List[List[TemplateMatchResult]]:
        """``predict`` on every window (x, y, w, h) of ``frame``, boxes relative to the window (base.py:238-253).  A matcher
        that batches over the windows overrides this."""
        return [self.predict(frame[y:y + h, x:x + w], template_frames, template_boxes, template_labels, template_texts,
                             score_threshold, scoring_strategy, max_objects, words=words, word_boxes=word_boxes,
                             word_lines=word_lines) for x, y, w, h in windows]

    def run(self, frames: List[np.ndarray], template_frames: List[np.ndarray], template_boxes: List[Sequence[int]],
            template_labels: List[str], template_texts: Optional[List[str]] = None, metadata=None,
            score_threshold: float = 0.90, scoring_strategy: str = "weighted", max_overlap: float = 0.5,
            max_objects: int = 1, window_size: Tuple[int, int] = (384, 128), regions=None, downscale_factor: float = 1.0,
            batch_size: Optional[int] = None) -> List[TemplateMatchResult]:
        """base.py:70-377: slice every frame into windows of ``window_size`` (h, w), match every window, shift the boxes to
        the page, keep scores above the threshold, merge overlapping boxes per label."""
        if not (0 <= score_threshold <= 1):
            raise ValueError("Score threshold should be between 0 and 1")
        if not (0 <= max_overlap <= 1):
            raise ValueError("Max overlap should be between 0 and 1")
        if not max_objects > 0:
            raise ValueError("Max object should be greater than 0")
        if downscale_factor > 1 or downscale_factor < 0:
            raise ValueError("Downscale factor should be between 0 and 1")
        if batch_size is not None and not batch_size > 0:
            raise ValueError("Batch size should be either None or greater than 0")
        if regions is None:
            regions = [(0, 0, image.shape[1], image.shape[0]) for image in frames]
        if len(frames) != len(regions):
            raise ValueError("The length of the regions list should be the same as the length of the frames list.")
        if downscale_factor != 1:
            raise NotImplementedError("downscale_factor != 1 needs resize_image_progressive, which is not built")
        results = []
        postprocess = self.setup_postprocess()
        for template_frame in template_frames:
            if template_frame.shape[0] != window_size[0] or template_frame.shape[1] != window_size[1]:
                raise ValueError("Template frame size does not match window size, please resize the template frames to "
                                 "match the window size")
        for frame_idx, frame in enumerate(frames):
            if frame.ndim != 3:
                raise ValueError(f"expected HxWx3 frames, got {frame.shape}")
            if self.slicing_enabled:
                windows = slice_image(frame.shape[0], frame.shape[1], window_size[0], window_size[1],
                                      self.DEFAULT_OVERLAP_HEIGHT_RATIO, self.DEFAULT_OVERLAP_WIDTH_RATIO)
            else:
                windows = [(0, 0, frame.shape[1], frame.shape[0])]
            words = word_boxes = word_lines = None
            if metadata:                                           # base.py:179-186; empty metadata counts as none
                words, word_boxes, word_lines = get_words_and_boxes(metadata, frame_idx, include_lines=True)
            per_window = self.predict_windows(frame, windows, template_frames, template_boxes, template_labels,
                                              template_texts, score_threshold, scoring_strategy, max_objects, words=words,
                                              word_boxes=word_boxes, word_lines=word_lines)
            bboxes, labels, scores, snippets = [], [], [], []
            for (ox, oy, _, _), predictions in zip(windows, per_window):
                for p in predictions:
                    bboxes.append([p.bbox[0] + ox, p.bbox[1] + oy, p.bbox[2], p.bbox[3]])
                    labels.append(p.label)
                    scores.append(p.score)
                    snippets.append(None)
            bboxes, labels, scores = self.filter_scores(bboxes, labels, scores, snippets, score_threshold)
            order = sorted(range(len(scores)), key=lambda i: scores[i], reverse=True)
            predictions = [ObjectPrediction([bboxes[i][0], bboxes[i][1], bboxes[i][0] + bboxes[i][2],
                                             bboxes[i][1] + bboxes[i][3]], scores[i], labels[i]) for i in order]
            if postprocess is not None:
                predictions = postprocess(predictions)
            by_label = {}
            for p in predictions:
                by_label.setdefault(p.category, []).append(p)
            for label, members in by_label.items():
                for p in members:
                    results.append(TemplateMatchResult(bbox=p.to_xywh(), label=label, score=p.score, similarity=p.score,
                                                       frame_index=frame_idx))
        return results

    def setup_postprocess(self):
        return GreedyNMMPostprocess(match_threshold=0.5, match_metric="IOS", class_agnostic=False)

    def filter_scores(self, bboxes, labels, scores, snippets, score_threshold) -> Tuple[list, list, list]:
        """drop what does not score strictly above the threshold"""
        assert len(bboxes) == len(labels) == len(scores) == len(snippets)
        keep = [i for i, s in enumerate(scores) if s > score_threshold]
        return [bboxes[i] for i in keep], [labels[i] for i in keep], [scores[i] for i in keep]

    @staticmethod
    def extract_windows(image: np.ndarray, template_bboxes: List[Sequence[int]], window_size: Tuple[int, int],
                        allow_padding: bool = False) -> Tuple[List[np.ndarray], List[Tuple[int, int, int, int]]]:
        """base.py:551-615: a window of ``window_size`` (h, w) centred on every box (x, y, w, h), moved back inside the
        image, and the box relative to its window; a smaller image is padded white when ``allow_padding``."""
        windows, bboxes = [], []
        img_h, img_w = image.shape[:2]
        desired_h, desired_w = window_size
        if img_h < desired_h or img_w < desired_w:
            if not allow_padding:
                raise ValueError(f"Image size should be greater than the window size, expected {window_size} but got "
                                 f"{image.shape[:2]}")
            padded = np.full((max(img_h, desired_h), max(img_w, desired_w), image.shape[2]), 255, image.dtype)
            padded[:img_h, :img_w] = image
            image = padded
            img_h, img_w = image.shape[:2]
        for x_, y_, w_, h_ in template_bboxes:
            center_x, center_y = x_ + w_ // 2, y_ + h_ // 2
            x, y = max(0, center_x - desired_w // 2), max(0, center_y - desired_h // 2)
            if x + desired_w > img_w:
                x = img_w - desired_w
            if y + desired_h > img_h:
                y = img_h - desired_h
            window = image[y:y + desired_h, x:x + desired_w, :]
            if window.shape[0] != desired_h or window.shape[1] != desired_w:
                raise Exception("Template frame size does not match window size, please resize the template frames to "
                                "match the window size")
            windows.append(window)
            bboxes.append((center_x - x - w_ // 2, center_y - y - h_ // 2, w_, h_))
        return windows, bboxes


# ---------------------------------------------------------------------------------------------------- VQ-NNF, host side
def odd(f) -> int:
    return int(np.ceil(f)) // 2 * 2 + 1


def gauss_box_3x3(sigma: float = 2.0) -> np.ndarray:
    """get_gaussian_box_filter((3, 3), sigma) of gauss_haar_filters.py:58-76: a centred impulse through a Gaussian
    (scipy.ndimage.gaussian_filter, mode 'reflect', truncate 4.0), as fp32."""
    radius = int(4.0 * sigma + 0.5)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    wts = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    wts /= wts.sum()
    line = np.pad(np.array([0.0, 1.0, 0.0]), radius, mode="symmetric")
    g = np.array([np.dot(wts, line[i:i + 2 * radius + 1]) for i in range(3)])
    return np.outer(g, g).astype(np.float32)


def integral_taps(box: np.ndarray) -> np.ndarray:
    """convert_box_to_integral (utils.py:12-18) in fp32, over the taps' count (gauss_haar_filters.py:205-207)"""
    mult = np.array([[1, -1], [-1, 1]], np.float32)
    out = np.zeros((box.shape[0] + 1, box.shape[1] + 1), np.float32)
    for i in range(box.shape[0]):
        for j in range(box.shape[1]):
            out[i:i + 2, j:j + 2] += np.float32(box[i, j]) * mult
    return out / np.float32(out.size)


def filter_bank(t_rows: int, t_cols: int, n_scales: int = 3):
    """GaussHaarFilters(kernel_size=3, sigma=2, filters=1, n_scales=3) for a template of t_rows x t_cols: ``haar_1x`` is
    listed twice, so two equal filters per scale -> taps (F, 4, 4) fp32, dilation (F, 2), kernel (F, 2), weight (F,)."""
    taps1 = integral_taps(gauss_box_3x3(2.0))
    taps, dil, ker, wgt = [], [], [], []
    for scale in np.linspace(1, 1 / n_scales, n_scales):
        d = (int(t_rows * scale) // 3, int(t_cols * scale) // 3)
        if d[0] < 1 or d[1] < 1:
            raise ValueError(f"a {t_rows} x {t_cols} template is too small: a side below 9 gives a filter dilation of 0")
        for _ in range(2):
            taps.append(taps1)
            dil.append(d)
            ker.append((3 * d[0] + 1, 3 * d[1] + 1))
            wgt.append(float(scale))
    return np.stack(taps), np.asarray(dil, np.int64), np.asarray(ker, np.int64), np.asarray(wgt, np.float64)


def template_responses(labels: np.ndarray, n_codes: int, taps: np.ndarray, dil: np.ndarray, ker: np.ndarray) -> np.ndarray:
    """GaussHaarFilters.get_template_features: the filters on the double cumulative sum of the one-hot of ``labels``
    (t_rows, t_cols), reflect-padded where a kernel exceeds the template, at the (1, 1) centre crop -> fp32 (F, K)."""
    onehot = (np.asarray(labels)[None, :, :] == np.arange(n_codes)[:, None, None]).astype(np.float64)
    integral = onehot.cumsum(axis=1).cumsum(axis=2)
    out = np.zeros((len(taps), n_codes), np.float64)
    for f in range(len(taps)):
        px = max(0, int(np.ceil((ker[f][0] - integral.shape[1]) / 2)))
        py = max(0, int(np.ceil((ker[f][1] - integral.shape[2]) / 2)))
        pad = np.pad(integral, ((0, 0), (px, px), (py, py)), mode="reflect")
        dx, dy = int(dil[f][0]), int(dil[f][1])
        hv, wv = pad.shape[1] - 3 * dx, pad.shape[2] - 3 * dy
        x1, y1 = ((hv - 1) // 2 if hv > 1 else 0), ((wv - 1) // 2 if wv > 1 else 0)
        for a in range(4):
            for b in range(4):
                out[f] += float(taps[f][a, b]) * pad[:, x1 + a * dx, y1 + b * dy]
    return out.astype(np.float32)


def peak_box(row: int, col: int, box_w: int, box_h: int) -> Tuple[int, int, int, int]:
    """vqnnf_template_matching.py:184-202 with its swapped names folded: the box (x, y, w, h) of a heat-map peak"""
    return (int(col + 1 - (odd(box_w) - 1) / 2), int(row + 1 - (odd(box_h) - 1) / 2), int(box_w), int(box_h))


def make_filters(taps, dil, wgt) -> VqFilters:
    fb = VqFilters()
    fb.n = len(taps)
    for f in range(len(taps)):
        for k, v in enumerate(np.asarray(taps[f], np.float32).reshape(-1)):
            fb.taps[f][k] = float(v)
        fb.dil[f][0], fb.dil[f][1] = int(dil[f][0]), int(dil[f][1])
        fb.weight[f] = float(wgt[f])
    return fb


def _u8(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.uint8)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


# ---- the kernels on host arrays (what tests/test_vqnnf_gpu.py drives)
def vq_assign_host(ctx: Context, image: np.ndarray, rect: Sequence[int], codebook: np.ndarray) -> np.ndarray:
    image, cb = _u8(image), np.ascontiguousarray(codebook, np.float32)
    r = np.asarray(rect, np.int32)
    out = np.empty((int(r[3]), int(r[2])), np.uint8)
    check(ctx.h, ctx.lib.mhip_vq_assign_host(ctx.h, _ptr(image), image.shape[0], image.shape[1], _ptr(r), _ptr(cb),
                                             cb.shape[0], _ptr(out)), "mhip_vq_assign_host")
    return out


def vq_kmeans_step_host(ctx: Context, image: np.ndarray, rect: Sequence[int], centroids: np.ndarray):
    """-> (labels uint8 (h*w,), new centroids fp32 (K, 27), members int32 (K,), error)"""
    image, cin = _u8(image), np.ascontiguousarray(centroids, np.float32)
    r = np.asarray(rect, np.int32)
    labels = np.empty(int(r[2]) * int(r[3]), np.uint8)
    cout, counts, err = np.empty_like(cin), np.empty(cin.shape[0], np.int32), C.c_double()
    check(ctx.h, ctx.lib.mhip_vq_kmeans_step_host(ctx.h, _ptr(image), image.shape[0], image.shape[1], _ptr(r), _ptr(cin),
                                                  cin.shape[0], _ptr(labels), _ptr(cout), _ptr(counts), C.byref(err)),
          "mhip_vq_kmeans_step_host")
    return labels, cout, counts, err.value


def vq_heatmap_host(ctx: Context, codes: np.ndarray, n_codes: int, responses: np.ndarray, taps, dil, wgt):
    """-> (heat fp32 (H, W), each filter's minimum fp64 (F,))"""
    codes, resp = _u8(codes), np.ascontiguousarray(responses, np.float32)
    fb = make_filters(taps, dil, wgt)
    heat, mins = np.empty(codes.shape, np.float32), np.empty(len(taps), np.float64)
    check(ctx.h, ctx.lib.mhip_vq_heatmap_host(ctx.h, _ptr(codes), codes.shape[0], codes.shape[1], int(n_codes), _ptr(resp),
                                              C.byref(fb), _ptr(heat), _ptr(mins)), "mhip_vq_heatmap_host")
    return heat, mins


def vq_peaks_host(ctx: Context, heat: np.ndarray, box_wh: Sequence[Sequence[int]], max_objects: int):
    """heat (n, H, W) -> (peaks fp32 (n, max_objects, 3) = row, col, value; the maps after the suppressions)"""
    heat = np.array(heat, np.float32, order="C", copy=True)
    wh = np.ascontiguousarray(box_wh, np.int32)
    peaks = np.empty((heat.shape[0], int(max_objects), 3), np.float32)
    check(ctx.h, ctx.lib.mhip_vq_peaks_host(ctx.h, _ptr(heat), heat.shape[0], heat.shape[1], heat.shape[2], _ptr(wh),
                                            int(max_objects), _ptr(peaks)), "mhip_vq_peaks_host")
    return peaks, heat


def clip_cosine_host(ctx: Context, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """cosine similarity of the colour features of clip pairs, uint8 (n, h, w, 3) each -> fp32 (n,)"""
    a, b = _u8(a), _u8(b)
    if a.shape != b.shape or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f"clip pairs of one (n, h, w, 3) shape expected, got {a.shape} and {b.shape}")
    out = np.empty(a.shape[0], np.float32)
    check(ctx.h, ctx.lib.mhip_clip_cosine_host(ctx.h, _ptr(a), _ptr(b), a.shape[0], a.shape[1], a.shape[2], _ptr(out)),
          "mhip_clip_cosine_host")
    return out


class VQTemplate:
    """``mhip_vq_template``: codebook, labels and filter responses of one template (frame + box) on a :class:`Context`."""

    def __init__(self, ctx: Context, frame, box: Sequence[int], init_idx: np.ndarray):
        """``frame``: an HxWx3 uint8 array, or a device tensor of that shape"""
        x, y, w, h = (int(v) for v in box)
        self.box = (x, y, w, h)
        taps, dil, ker, wgt = filter_bank(h, w)                    # ValueError for a side below 9, before any launch
        self.ctx, self.lib = ctx, ctx.lib
        on_device = hasattr(frame, "data_ptr")
        if not on_device:
            frame = _u8(frame)
        fh, fw = int(frame.shape[0]), int(frame.shape[1])
        idx = np.ascontiguousarray(init_idx, np.int32)
        b = np.asarray(self.box, np.int32)
        handle = C.c_void_p()
        check(ctx.h, self.lib.mhip_vq_template_create(ctx.h, C.c_void_p(frame.data_ptr()) if on_device else _ptr(frame),
                                                      1 if on_device else 0, fh, fw, _ptr(b), _ptr(idx), len(idx),
                                                      C.byref(handle)), "mhip_vq_template_create")
        self.h = handle
        ctx.adopt(self)
        k, it = C.c_int(), C.c_int()
        self.lib.mhip_vq_template_state(self.h, C.byref(k), C.byref(it), None, None)
        self.n_codes, self.iterations = k.value, it.value
        self.labels = np.empty(w * h, np.uint8)
        self.codebook = np.empty((self.n_codes, N_FEATURES), np.float32)
        self.lib.mhip_vq_template_state(self.h, None, None, _ptr(self.labels), _ptr(self.codebook))
        self.taps, self.dil, self.ker, self.wgt = taps, dil, ker, wgt
        self.responses = template_responses(self.labels.reshape(h, w), self.n_codes, taps, dil, ker)
        fb = make_filters(taps, dil, wgt)
        check(ctx.h, self.lib.mhip_vq_template_set_filters(self.h, _ptr(self.responses), C.byref(fb)),
              "mhip_vq_template_set_filters")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.mhip_vq_template_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def n_code_of(w: int, h: int, n_code: int = N_CODE) -> int:
    """template_matching.py:46-48"""
    return n_code if w * h > n_code else w * h


def draw_init_indices(seed: int, box: Sequence[int]) -> np.ndarray:
    """the rows init_methods._kpoints draws (with replacement), from a generator seeded by (seed, box)"""
    x, y, w, h = (int(v) for v in box)
    rng = np.random.default_rng([int(seed), x, y, w, h])
    return rng.integers(0, w * h, size=n_code_of(w, h)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- snippet scoring
# What VQNNFTemplateMatcher.score and MetaTemplateMatcher.score share: the embedding of 224 x 224 snippet clips, cached by the
# clips' bytes (``cached_embeddings_clips`` of either matcher), and the cosine of (template clip, query clip) pairs.
def is_embeddings_object(processor) -> bool:
    """an embeddings object of embeddings.py (batched device entries), not a plain callable clip -> vector"""
    return hasattr(processor, "cosine_pairs")


def host_cosine(a: np.ndarray, b: np.ndarray):
    """nn.CosineSimilarity of two vectors: each norm clamped at 1e-8"""
    return np.dot(a, b) / (max(np.linalg.norm(a), 1e-8) * max(np.linalg.norm(b), 1e-8))


def clip_embedding(processor, cache: dict, clip: np.ndarray) -> np.ndarray:
    """the embedding of one clip, through ``cache``"""
    key = clip.tobytes()
    if key not in cache:
        if clip.shape[0] != CLIP_SIZE[0] or clip.shape[1] != CLIP_SIZE[1]:
            raise ValueError("Image must be 224x224")
        if is_embeddings_object(processor):
            cache[key] = processor.embed_clips(clip[None])[0]
        else:
            cache[key] = np.asarray(processor(clip), np.float64).reshape(-1)
    return cache[key]


def clip_embedding_sims(ep, cache: dict, t_clips: Sequence[np.ndarray], q_clips: Sequence[np.ndarray]) -> np.ndarray:
    """The embedding cosine of every (template clip, query clip) pair through an embeddings object: the unique clips of
    the batch, keyed by their bytes as ``cache`` is, take one encoder call and the cosines one launch.
    Clips embedded by an earlier batch (the templates of the previous page) are not embedded again."""
    index, clips = {}, []
    for clip in list(t_clips) + list(q_clips):
        key = clip.tobytes()
        if key not in index:
            if clip.shape[0] != CLIP_SIZE[0] or clip.shape[1] != CLIP_SIZE[1]:
                raise ValueError("Image must be 224x224")
            index[key] = len(clips)
            clips.append(clip)
    pairs = [(index[t.tobytes()], index[q.tobytes()]) for t, q in zip(t_clips, q_clips)]
    keys = list(index)
    new = [i for i, key in enumerate(keys) if key not in cache]
    if len(new) == len(keys):                      # nothing known yet: encoder and cosines in one call
        sims, emb = ep.cosine_pairs(np.stack(clips), pairs, want_embeddings=True)
        cache.update(zip(keys, emb))
        return sims
    if new:
        cache.update(zip((keys[i] for i in new), ep.embed_clips(np.stack([clips[i] for i in new]))))
    return ep.pair_cosines(np.stack([cache[key] for key in keys]), pairs)


# ---------------------------------------------------------------------------------------------------- the matcher
class VQNNFTemplateMatcher(BaseTemplateMatcher):
    """Drop-in for marie/components/template_matching/vqnnf_template_matching.py on the colour features."""

    def __init__(self, model_name_or_path: Union[str, os.PathLike] = "", model_version: Optional[str] = None,
                 use_gpu: bool = True, labels: Optional[List[str]] = None, batch_size: int = 16, use_auth_token=None,
                 devices: Optional[List[Any]] = None, show_error: Optional[Union[str, bool]] = True, *,
                 n_feature: int = N_FEATURES, pca_dims: Optional[int] = None,
                 embeddings_processor: Union[Callable[[np.ndarray], np.ndarray], Any, None] = None, seed: int = 0,
                 ctx: Optional[Context] = None, **kwargs):
        super().__init__(True, **kwargs)
        if not use_gpu:
            raise MarieHipError("VQNNFTemplateMatcher here is the MI355X path; use_gpu=False has no implementation")
        if n_feature != N_FEATURES:
            raise NotImplementedError("n_feature != 27: the EfficientNet hyper-column features are not built")
        if pca_dims is not None:
            raise NotImplementedError("pca_dims: the pca_lowrank projection of the features is not built")
        logger.info("VQNNF matcher model : %s", model_name_or_path)
        self.show_error, self.batch_size, self.labels = show_error, batch_size, labels
        self.n_feature, self.n_code, self.seed = n_feature, N_CODE, int(seed)
        self.embeddings_processor = embeddings_processor
        self.ctx = ctx or Context(self._device_id(devices))
        self.cached_features = {}            # key_{x}_{y}_{w}_{h} -> VQTemplate
        self.cached_embeddings_clips = {}
        self.template_builds = 0             # k-means runs so far

    @staticmethod
    def _device_id(devices) -> int:
        if not devices:
            return 0
        d = devices[0]
        idx = getattr(d, "index", None)
        if idx is None and isinstance(d, str) and ":" in d:
            idx = int(d.split(":")[1])
        return int(idx or 0)

    def close(self):
        for t in self.cached_features.values():
            t.close()
        self.cached_features = {}

    # -- template state ----------------------------------------------------------------------------------------------
    def template_state(self, template_frame: np.ndarray, template_box: Sequence[int]) -> VQTemplate:
        x, y, w, h = (int(t) for t in template_box)
        key = f"key_{x}_{y}_{w}_{h}"
        if key not in self.cached_features:
            box = (max(x, 0), max(y, 0), w, h)
            self.cached_features[key] = VQTemplate(self.ctx, template_frame, box, draw_init_indices(self.seed, box))
            self.template_builds += 1
        return self.cached_features[key]

    # -- device matching ---------------------------------------------------------------------------------------------
    def match_windows(self, frame: np.ndarray, windows: Sequence[Sequence[int]], template_frames, template_boxes,
                      max_objects: int) -> np.ndarray:
        """Every window (x, y, w, h; one size) of ``frame`` against every template in one batched call ->
        peaks fp32 (n_windows, n_templates, max_objects, 3) = row, col, value of the heat-map maxima."""
        import torch

        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 frame, got {frame.shape}")
        sizes = {(int(w[2]), int(w[3])) for w in windows}
        if len(sizes) != 1:
            raise ValueError(f"the windows of one call share one size, got {sorted(sizes)}")
        win_w, win_h = sizes.pop()
        states = [self.template_state(f, b) for f, b in zip(template_frames, template_boxes)]
        dev_name = f"cuda:{self.ctx.device_id}"
        self.ctx.set_stream(torch.cuda.current_stream(dev_name).cuda_stream)
        page = torch.from_numpy(_u8(frame)).to(dev_name)
        xy = np.ascontiguousarray([[int(w[0]), int(w[1])] for w in windows], np.int32)
        handles = (C.c_void_p * len(states))(*[s.h.value for s in states])
        peaks = np.empty((len(windows), len(states), int(max_objects), 3), np.float32)
        check(self.ctx.h, self.ctx.lib.mhip_vq_match(self.ctx.h, C.c_void_p(page.data_ptr()), frame.shape[0], frame.shape[1],
                                                     frame.shape[1] * 3, _ptr(xy), len(windows), win_h, win_w, handles,
                                                     len(states), int(max_objects), _ptr(peaks)), "mhip_vq_match")
        return peaks

    # -- scoring -----------------------------------------------------------------------------------------------------
    def _clip(self, snippet: np.ndarray) -> np.ndarray:
        return _u8(resize_image(_u8(snippet), CLIP_SIZE, ctx=self.ctx)[0])

    def get_embedding_feature(self, clip: np.ndarray) -> np.ndarray:
        return clip_embedding(self.embeddings_processor, self.cached_embeddings_clips, clip)

    def _batched_embeddings(self) -> bool:
        return is_embeddings_object(self.embeddings_processor)

    def embedding_sims(self, t_clips: np.ndarray, q_clips: np.ndarray) -> np.ndarray:
        return clip_embedding_sims(self.embeddings_processor, self.cached_embeddings_clips, t_clips, q_clips)

    def score_pairs(self, pairs: Sequence[Tuple[np.ndarray, np.ndarray]], scoring_strategy: str) -> List[float]:
        """``score`` of (template snippet, query snippet) pairs with one cosine launch for all of them"""
        if not pairs:
            return []
        t_clips = np.stack([self._clip(t) for t, _ in pairs])
        q_clips = np.stack([self._clip(q) for _, q in pairs])
        feature_sims = clip_cosine_host(self.ctx, t_clips, q_clips)
        batched = self.embedding_sims(t_clips, q_clips) if self._batched_embeddings() else None
        out = []
        for k, feature_sim in enumerate(feature_sims):
            feature_sim = float(feature_sim)
            if self.embeddings_processor is None:
                embedding_sim = feature_sim
            elif batched is not None:
                embedding_sim = float(batched[k])
            else:
                embedding_sim = float(host_cosine(self.get_embedding_feature(t_clips[k]), self.get_embedding_feature(q_clips[k])))
            if scoring_strategy == "weighted":
                sim_val = feature_sim * 0.05 + embedding_sim * 0.95
            elif scoring_strategy == "max":
                sim_val = max(feature_sim, embedding_sim)
            else:
                sim_val = (feature_sim + embedding_sim) / 2
            out.append(max(0, min(1, sim_val)))
        return out

    def score(self, template_snippet: np.ndarray, query_pred_snippet: np.ndarray, scoring_strategy: str) -> float:
        """vqnnf_template_matching.py:310-362"""
        return self.score_pairs([(template_snippet, query_pred_snippet)], scoring_strategy)[0]

    # -- predictions -------------------------------------------------------------------------------------------------
    def predict_windows(self, frame, windows, template_frames, template_boxes, template_labels, template_texts=None,
                        score_threshold: float = 0.9, scoring_strategy: str = "weighted", max_objects: int = 1, words=None,
                        word_boxes=None, word_lines=None) -> List[List[TemplateMatchResult]]:
        peaks = self.match_windows(frame, windows, template_frames, template_boxes, max_objects)
        candidates, pairs = [], []            # (window, template, k, box) of every peak with a snippet, in the loop's order
        for wi, (wx, wy, ww, wh) in enumerate(windows):
            patch = frame[wy:wy + wh, wx:wx + ww]
            for ti, (tframe, tbox) in enumerate(zip(template_frames, template_boxes)):
                tx, ty = int(max(tbox[0], 0)), int(max(tbox[1], 0))
                tw, th = int(tbox[2]), int(tbox[3])
                template_snippet = tframe[ty:min(ty + th, tframe.shape[0]), tx:min(tx + tw, tframe.shape[1])]
                for k in range(max_objects):
                    box = peak_box(int(peaks[wi, ti, k, 0]), int(peaks[wi, ti, k, 1]), tw, th)
                    snippet = patch[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
                    if template_snippet.shape[0] == 0 or template_snippet.shape[1] == 0:
                        logger.warning("Template snippet is empty")
                        continue
                    if snippet.shape[0] == 0 or snippet.shape[1] == 0:
                        logger.warning("Query snippet is empty")
                        continue
                    candidates.append((wi, ti, k, box))
                    pairs.append((template_snippet, snippet))
        scores = self.score_pairs(pairs, scoring_strategy)
        out: List[List[TemplateMatchResult]] = [[] for _ in windows]
        stopped = set()                       # the reference's break at the first candidate under the threshold
        for (wi, ti, k, box), sim_val in zip(candidates, scores):
            if (wi, ti) in stopped:
                continue
            if sim_val < score_threshold:
                stopped.add((wi, ti))
                continue
            out[wi].append(TemplateMatchResult(bbox=box, label=template_labels[ti], score=sim_val, similarity=sim_val,
                                               frame_index=-1))
        return out

    def predict(self, frame, template_frames, template_boxes, template_labels, template_texts=None,
                score_threshold: float = 0.9, scoring_strategy: str = "weighted", max_objects: int = 1, batch_size: int = 1,
                words=None, word_boxes=None, word_lines=None) -> List[TemplateMatchResult]:
        """vqnnf_template_matching.py:100-308 on one frame (the whole frame is the window)"""
        return self.predict_windows(frame, [(0, 0, frame.shape[1], frame.shape[0])], template_frames, template_boxes,
                                    template_labels, template_texts, score_threshold, scoring_strategy, max_objects)[0]


# ---------------------------------------------------------------------------------------------------- text matching
LEV_MAX_PATTERN = 1024             # code points of a template text (csrc/lev_ngrams.hip: LEV_MAX_M)
LEV_LDS_BYTES = 65536              # the kernel's budget for a template's bit table (LEV_LDS_BYTES there)


def is_overlap(bbox1, bbox2) -> bool:
    """meta_template_matching.py:23-30, boxes as (x, y, w, h)"""
    x1, y1, w1, h1 = bbox1
    x2, y2, w2, h2 = bbox2
    return bool(x1 < x2 + w2 and x1 + w1 > x2 and y1 < y2 + h2 and y1 + h1 > y2)


def _code_points(text: str) -> np.ndarray:
    return np.frombuffer(text.encode("utf-32-le", "surrogatepass"), np.uint32)


@dataclass
class TextLayout:
    """A page's words and the template texts as the edit-distance kernel takes them (``text_layout``)."""
    text: str                  # S: the upper-cased words joined by blanks
    page_ids: np.ndarray       # uint16 (L,): the alphabet id of every code point of S, 0 for one outside the alphabet
    ws: np.ndarray             # int32 (N,): word i is S[ws[i]:we[i]]
    we: np.ndarray
    fs: np.ndarray             # int32 (N,): first position >= ws[i] of S that is not white space (L: none)
    le: np.ndarray             # int32 (N,): one past the last position < we[i] of S that is not white space (0: none)
    alphabet: int              # A: ids 1 .. A are the code points of the patterns
    pattern_ids: np.ndarray    # uint16: the patterns' ids, concatenated
    pattern_off: np.ndarray    # int32 (T + 1,)

    def span(self, i: int, n: int) -> Tuple[int, int]:
        """(a, b): S[a:b] == " ".join(words[i:i + n]).strip().upper()"""
        a = min(int(self.fs[i]), int(self.we[i + n - 1]))
        return a, max(int(self.le[i + n - 1]), a)


def text_layout(words: Sequence[str], patterns: Sequence[str], raw: bool = False) -> TextLayout:
    """The host side of ``mhip_lev_ngrams_host``.  ``upper()`` acts per character and ``strip()`` only moves the two ends, so every
    n-gram string of the reference is a substring of ONE string S; the strip is precomputed per word (white space as
    ``str.isspace``, which can run through empty or blank words into their neighbours).  Distances are over code points: S is
    handled as UTF-32, so an astral character counts once.  ``patterns``: the stripped, upper-cased template texts.
    ``raw``: the words as they are, neither upper-cased nor stripped."""
    upper = list(words) if raw else [w.upper() for w in words]
    text = " ".join(upper)
    cp = _code_points(text)
    L, N = len(cp), len(upper)
    lens = np.fromiter((len(u) for u in upper), np.int64, N)
    we = np.cumsum(lens + 1) - 1
    ws = we - lens
    uniq, inverse = np.unique(cp, return_inverse=True)
    space = np.fromiter((chr(u).isspace() for u in uniq), bool, len(uniq))[inverse.reshape(-1)] if L else np.zeros(0, bool)
    ink = np.flatnonzero(~space)                                   # the positions strip() stops at
    before = np.searchsorted(ink, ws, "left")                      # ink positions before ws[i]: the next one is fs[i]
    fs = np.append(ink, L)[before]
    le = np.insert(ink, 0, -1)[np.searchsorted(ink, we, "left")] + 1
    if raw:
        fs, le = ws, we
    pats = [_code_points(p) for p in patterns]
    letters = np.unique(np.concatenate(pats)) if pats and sum(len(p) for p in pats) else np.zeros(0, np.uint32)
    if len(letters) > 65535:
        raise ValueError(f"the template texts hold {len(letters)} distinct code points; ids are 16 bits")

    def ids(points):
        if not len(letters) or not len(points):
            return np.zeros(len(points), np.uint16)
        at = np.minimum(np.searchsorted(letters, points), len(letters) - 1)
        return np.where(letters[at] == points, at + 1, 0).astype(np.uint16)

    off = np.zeros(len(pats) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in pats])
    pattern_ids = np.concatenate([ids(p) for p in pats]) if pats else np.zeros(0, np.uint16)
    return TextLayout(text, ids(cp), ws.astype(np.int32), we.astype(np.int32), fs.astype(np.int32), le.astype(np.int32),
                      len(letters), pattern_ids.astype(np.uint16), off)


def lev_ngrams_host(ctx: Context, layout: TextLayout, g: Sequence[int], line_ids: Optional[Sequence[int]] = None):
    """The edit distance of every pattern of ``layout`` against every n-gram of g[t] - 1, g[t] and g[t] + 1 words, one call ->
    (dist, len) int32 (T, 3, N): the distance and the candidate's length in code points, -1 where there is no candidate.
    ``line_ids`` (one int per word): a candidate whose words do not share one id is none."""
    T, N = len(layout.pattern_off) - 1, len(layout.ws)
    g = np.ascontiguousarray(g, np.int32)
    if T < 1 or N < 1 or len(g) != T:
        raise ValueError(f"lev_ngrams: {T} patterns with {len(g)} word counts over {N} words")
    m = np.diff(layout.pattern_off)
    if m.max() > LEV_MAX_PATTERN:
        raise ValueError(f"a template text of {int(m.max())} code points: at most {LEV_MAX_PATTERN} are built")
    table = (layout.alphabet + 1) * ((int(m.max()) + 63) // 64) * 8
    if table > LEV_LDS_BYTES:
        raise ValueError(f"a template text of {int(m.max())} code points over an alphabet of {layout.alphabet} needs a bit table "
                         f"of {table} bytes; {LEV_LDS_BYTES} are budgeted")
    lines = None
    if line_ids is not None:
        lines = np.ascontiguousarray(line_ids, np.int32)
        if lines.shape != (N,):
            raise ValueError(f"lev_ngrams: {lines.shape} line ids for {N} words")
    page, pat, off = (np.ascontiguousarray(layout.page_ids, np.uint16), np.ascontiguousarray(layout.pattern_ids, np.uint16),
                      np.ascontiguousarray(layout.pattern_off, np.int32))
    arrays = [np.ascontiguousarray(a, np.int32) for a in (layout.ws, layout.we, layout.fs, layout.le)]
    dist, length = np.empty((T, 3, N), np.int32), np.empty((T, 3, N), np.int32)
    check(ctx.h, ctx.lib.mhip_lev_ngrams_host(ctx.h, _ptr(page), len(page), *[_ptr(a) for a in arrays],
                                              _ptr(lines) if lines is not None else None, N, _ptr(pat), _ptr(off), _ptr(g), T,
                                              int(layout.alphabet), _ptr(dist), _ptr(length)), "mhip_lev_ngrams_host")
    return dist, length


@dataclass
class MetaCandidate:
    """one (template, n-gram) pair of ``MetaTemplateMatcher`` with the unrounded terms of its score"""
    template: int              # index into the template lists
    ngram: int                 # words of the n-gram
    start: int                 # its first word
    words: str                 # " ".join(words[start:start + ngram]).strip().upper()
    bbox: Any                  # merge_bboxes_as_block of the words' boxes
    lev: float
    cos_text: Optional[float]  # None below lev 0.5: the reference returns lev alone there
    cos_image: Optional[float]
    total: float


class MetaTemplateMatcher(BaseTemplateMatcher):
    """Drop-in for marie/components/template_matching/meta_template_matching.py: the template's text among the page's words."""

    MIN_WORD_LENGTH = 3
    MAX_TEXT_LENGTH = 1024        # get_embedding cuts a text there

    def __init__(self, model_name_or_path: Union[str, os.PathLike] = "", model_version: Optional[str] = None,
                 use_gpu: bool = True, labels: Optional[List[str]] = None, batch_size: int = 16, use_auth_token=None,
                 devices: Optional[List[Any]] = None, show_error: Optional[Union[str, bool]] = True, *,
                 embeddings_processor: Union[Callable[[np.ndarray], np.ndarray], Any, None] = None,
                 text_embeddings_processor: Union[Callable[[str], np.ndarray], Any, None] = None,
                 ctx: Optional[Context] = None, **kwargs):
        """``embeddings_processor``: an embeddings object of ``embeddings.py`` (its vision tower scores the snippets, its text
        tower the texts) or a callable clip -> vector.  ``text_embeddings_processor``: an embeddings object with a text side, or
        a callable text -> vector; needed when ``embeddings_processor`` has no text side."""
        super().__init__(False, **kwargs)
        if not use_gpu:
            raise MarieHipError("MetaTemplateMatcher here is the MI355X path; use_gpu=False has no implementation")
        if embeddings_processor is None:
            raise ValueError("MetaTemplateMatcher needs an embeddings_processor for the snippet score")
        if text_embeddings_processor is None:
            if getattr(embeddings_processor, "text_model", None) is None:
                raise ValueError("MetaTemplateMatcher needs text embeddings: embeddings_processor has no text side and no "
                                 "text_embeddings_processor is given")
            text_embeddings_processor = embeddings_processor
        elif hasattr(text_embeddings_processor, "embed_texts") and getattr(text_embeddings_processor, "text_model", None) is None:
            raise ValueError("MetaTemplateMatcher: text_embeddings_processor has no text side")
        logger.info("Document matcher : %s", model_name_or_path)
        self.show_error, self.batch_size, self.labels = show_error, batch_size, labels
        self.embeddings_processor = embeddings_processor
        self.text_embeddings_processor = text_embeddings_processor
        self.ctx = ctx or getattr(embeddings_processor, "ctx", None) or Context(VQNNFTemplateMatcher._device_id(devices))
        self.embedding_cache = {}             # text -> embedding
        self.cached_embeddings_clips = {}     # clip bytes -> embedding

    # -- embeddings ----------------------------------------------------------------------------------------------------
    def _clip(self, snippet: np.ndarray) -> np.ndarray:
        if snippet.shape[0] == 0 or snippet.shape[1] == 0:
            raise ValueError(f"an empty snippet {snippet.shape}: the box lies outside its frame")
        return _u8(resize_image(_u8(snippet), CLIP_SIZE, ctx=self.ctx)[0])

    def image_sims(self, t_clips: Sequence[np.ndarray], q_clips: Sequence[np.ndarray]) -> List[float]:
        ep, cache = self.embeddings_processor, self.cached_embeddings_clips
        if is_embeddings_object(ep):
            return [float(v) for v in clip_embedding_sims(ep, cache, t_clips, q_clips)]
        return [float(host_cosine(clip_embedding(ep, cache, t), clip_embedding(ep, cache, q))) for t, q in zip(t_clips, q_clips)]

    def text_sims(self, pairs: Sequence[Tuple[str, str]]) -> List[float]:
        """the cosine of the embeddings of (n-gram text, template text) pairs; ``embedding_cache`` is keyed by the whole text,
        the embedding is of its first 1024 characters (meta_template_matching.py:239-247)"""
        ep, cache = self.text_embeddings_processor, self.embedding_cache
        new = list(dict.fromkeys(t for pair in pairs for t in pair if t not in cache))
        if not hasattr(ep, "embed_texts"):                         # a callable text -> vector
            for t in new:
                cache[t] = np.asarray(ep(t[:self.MAX_TEXT_LENGTH]), np.float64).reshape(-1)
            return [float(host_cosine(cache[a], cache[b])) for a, b in pairs]
        if new:
            cache.update(zip(new, ep.embed_texts([t[:self.MAX_TEXT_LENGTH] for t in new], truncation=True)))
        index = {t: k for k, t in enumerate(dict.fromkeys(t for pair in pairs for t in pair))}
        return [float(v) for v in ep.pair_cosines(np.stack([cache[t] for t in index]), [(index[a], index[b]) for a, b in pairs])]

    # -- scoring -------------------------------------------------------------------------------------------------------
    def _candidates(self, frame, template_frames, template_boxes, template_texts, words, word_boxes, word_lines,
                    keep_from: float) -> List[MetaCandidate]:
        """Every (template, n-gram) pair whose Levenshtein similarity is at least ``min(keep_from, 0.5)``, scored, in the
        reference's order: template, n-gram size, first word."""
        used = [k for k, text in enumerate(template_texts) if text is not None and len(text) >= self.MIN_WORD_LENGTH]
        if not used or not len(words):
            return []
        patterns = [template_texts[k].strip().upper() for k in used]
        layout = text_layout(words, patterns)
        g = [len(template_texts[k].split(" ")) for k in used]
        line_ids = None
        if word_lines:
            seen = {}
            line_ids = [seen.setdefault(line, len(seen)) for line in word_lines]
        dist, length = lev_ngrams_host(self.ctx, layout, g, line_ids)
        m = np.diff(layout.pattern_off).astype(np.int64)[:, None, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            lev = 1 - dist / np.maximum(length, m)                   # double, as 1 - d / max(len_a, len_b) in Python
        if np.any((dist >= 0) & (np.maximum(length, m) == 0)):
            raise ZeroDivisionError("an empty n-gram against an empty template text")
        out, t_clips, q_clips, texts, scored = [], [], [], [], []
        fragments, snippets = {}, {}
        for t, k, i in zip(*np.nonzero((dist >= 0) & (lev >= min(keep_from, 0.5)))):
            n = g[t] - 1 + int(k)
            a, b = layout.span(int(i), n)
            box = merge_bboxes_as_block(word_boxes[i:i + n])
            c = MetaCandidate(used[t], n, int(i), layout.text[a:b], box, float(lev[t, k, i]), None, None, float(lev[t, k, i]))
            out.append(c)
            if c.lev < 0.5:
                continue
            if t not in fragments:
                tx, ty, tw, th = template_boxes[used[t]]
                tx, ty = int(max(tx, 0)), int(max(ty, 0))
                fragments[t] = self._clip(template_frames[used[t]][ty:ty + th, tx:tx + tw])
            key = tuple(box)
            if key not in snippets:
                x, y, w, h = box
                snippets[key] = self._clip(frame[y:y + h, x:x + w])
            scored.append(c)
            t_clips.append(fragments[t])
            q_clips.append(snippets[key])
            texts.append((c.words, patterns[t]))
        if scored:
            for c, cos_text, cos_image in zip(scored, self.text_sims(texts), self.image_sims(t_clips, q_clips)):
                c.cos_text, c.cos_image = cos_text, cos_image
                c.total = (c.lev + cos_text + cos_image) / 3
        return out

    def score_candidates(self, frame, template_frames, template_boxes, template_texts, words, word_boxes,
                         word_lines=None) -> List[MetaCandidate]:
        """The unrounded (lev, cos_text, cos_image, total) of every (template, n-gram) pair at a Levenshtein similarity of 0.5
        or more: what ``score`` (meta_template_matching.py:270-311) averages."""
        self._check(template_frames, template_boxes, template_texts, None, words, word_boxes)
        return [c for c in self._candidates(frame, template_frames, template_boxes, template_texts, words, word_boxes,
                                            word_lines, 0.5) if c.lev >= 0.5]

    def score(self, ngram_words: str, template_text: str, query_snippet: np.ndarray, template_snippet: np.ndarray) -> float:
        """meta_template_matching.py:270-311 for one pair"""
        d = int(lev_ngrams_host(self.ctx, text_layout([ngram_words], [template_text], raw=True), [1])[0][0, 1, 0])
        sim_val = 1 - d / max(len(ngram_words), len(template_text))
        if sim_val < 0.5:
            return sim_val
        cos_image = self.image_sims([self._clip(template_snippet)], [self._clip(query_snippet)])[0]
        cos_text = self.text_sims([(ngram_words, template_text)])[0]
        return (sim_val + cos_text + cos_image) / 3

    @staticmethod
    def _check(template_frames, template_boxes, template_texts, template_labels, words, word_boxes):
        if template_texts is None:
            raise ValueError("MetaTemplateMatcher matches template_texts; none were given")
        assert len(words) == len(word_boxes)
        assert len(template_frames) == len(template_boxes)
        assert template_labels is None or len(template_texts) == len(template_labels)

    def predict(self, frame, template_frames, template_boxes, template_labels, template_texts=None,
                score_threshold: float = 0.9, scoring_strategy: str = "weighted", max_objects: int = 1, batch_size: int = 1,
                words=None, word_boxes=None, word_lines=None) -> List[TemplateMatchResult]:
        """meta_template_matching.py:98-237"""
        predictions: List[TemplateMatchResult] = []
        if words is None or word_boxes is None:
            logger.warning("No words or word_boxes provided. Skipping prediction.")
            return predictions
        self._check(template_frames, template_boxes, template_texts, template_labels, words, word_boxes)
        scored = self._candidates(frame, template_frames, template_boxes, template_texts, words, word_boxes, word_lines,
                                  score_threshold - 0.001)      # round(x, 3) > threshold needs x > threshold - 0.0005
        by_template = {}
        for c in scored:
            sim_val = round(c.total, 3)
            if c.words == template_texts[c.template].strip().upper() or sim_val > score_threshold:
                by_template.setdefault(c.template, []).append((c.ngram, TemplateMatchResult(
                    bbox=c.bbox, label=template_labels[c.template], score=sim_val, similarity=sim_val)))
        for idx in sorted(by_template):
            for _, candidate in sorted(by_template[idx], key=lambda e: e[0]):          # stable: by n-gram size
                if not any(candidate.label == p.label and is_overlap(candidate.bbox, p.bbox) for p in predictions):
                    predictions.append(candidate)
        return predictions


class CompositeTemplateMatcher(BaseTemplateMatcher):
    """marie/components/template_matching/composite_template_maching.py: several matchers in turn, merged per page."""

    def __init__(self, matchers: List[BaseTemplateMatcher], break_on_match: bool = False,
                 show_error: Optional[Union[str, bool]] = True, embeddings_processor: Any = None, **kwargs):
        """``embeddings_processor``: handed to every matcher that scores with one and has none of its own"""
        super().__init__(False, **kwargs)
        self.show_error, self.matchers, self.break_on_match = show_error, matchers, break_on_match
        self.embeddings_processor = embeddings_processor
        if embeddings_processor is not None:
            for matcher in matchers:
                if hasattr(matcher, "embeddings_processor") and matcher.embeddings_processor is None:
                    matcher.embeddings_processor = embeddings_processor

    def predict(self, *args, **kwargs):
        raise NotImplementedError("This method is not implemented in CompositeTemplateMatcher")

    def run(self, frames, template_frames, template_boxes, template_labels, template_texts=None, metadata=None,
            score_threshold: float = 0.8, scoring_strategy: str = "weighted", max_overlap: float = 0.5, max_objects: int = 1,
            window_size: Tuple[int, int] = (384, 128), regions=None, downscale_factor: float = 1.0,
            batch_size: Optional[int] = None) -> List[TemplateMatchResult]:
        results = []
        postprocess = self.setup_postprocess()
        for matcher in self.matchers:
            result = matcher.run(frames=frames, template_frames=template_frames, template_boxes=template_boxes,
                                 template_labels=template_labels, template_texts=template_texts, metadata=metadata,
                                 score_threshold=score_threshold, scoring_strategy=scoring_strategy, max_overlap=max_overlap,
                                 max_objects=max_objects, window_size=window_size, regions=regions,
                                 downscale_factor=downscale_factor, batch_size=batch_size)
            results.extend(result)
            if self.break_on_match and result:
                break
        by_page = {}
        for r in results:
            by_page.setdefault(r.frame_index, []).append(r)
        converted = []
        for page_index, members in by_page.items():
            predictions = [ObjectPrediction([r.bbox[0], r.bbox[1], r.bbox[0] + r.bbox[2], r.bbox[1] + r.bbox[3]], r.score,
                                            r.label) for r in members]
            for p in postprocess(predictions):
                converted.append(TemplateMatchResult(bbox=p.to_xywh(), label=p.category, score=p.score, similarity=p.score,
                                                     frame_index=page_index))
        return converted
