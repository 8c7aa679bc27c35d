"""Document boundary registration on the MI355X: ``UnilmDocumentBoundaryRegistration`` and its no-op twin.

Mirrors marie/components/document_registration/{datamodel,base,unilm_dit}.py.  The reference runs a DiT Mask R-CNN with five
box classes (config/zoo/unilm/dit/object_detection/document_boundary/prod.yaml) on every frame, takes the document's box, crops
the page to it (plus margins) and re-places the crop at a fixed registration point — ``absolute`` (pasted on a white page) or
``fit_to_page`` (resized to the page width less the margins, then bordered) — with red registration markers, then resizes the
result back to the frame's shape (``debug_visualization`` is forced on in the reference's constructor, so that restore is what
production returns).

Here the detector is ``DitModel`` with :func:`marie_icr_amd.dit.boundary_config` (the K-class final stage of
csrc/det_ops.hip), and crop, resize, border, markers and the shape restore are one warp on the device page
(``mhip_register_warp``, csrc/ingest.hip).  Each page is uploaded once, detected in batches of pages of one size, warped from
the same device copy and downloaded once.  The choice of box and the geometry of the warp are :func:`registration_plan`, a pure
function of the detections.

Not reproduced: the detectron2 ``Visualizer`` image (``visualization_image`` is always None) and the reference's debug writes
under /tmp/dit and its prints.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from dataclasses import dataclass, field
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np
from pydantic import BaseModel, ConfigDict

from ._lib import PREC_F16, PREC_F32, Context, MarieHipError, RegisterDesc, check
from .dit import DitModel, boundary_config

logger = logging.getLogger(__name__)

MODEL_SUBPATH = "unilm/dit/object_detection/document_boundary/model_final.pth"
MIN_SCORE = 0.7                 # unilm_dit.py:378, when more than one box is predicted
MARKER_RADIUS = 8
MARKER_COLOR = (0, 0, 255)      # cv2.circle colour, array channel order


class DocumentBoundaryPrediction(BaseModel):
    """marie/components/document_registration/datamodel.py"""
    label: str
    detected: bool
    mode: str
    aligned_image: Union[np.ndarray, None] = None
    boundary_bbox: List[int]
    score: float
    visualization_image: Union[np.ndarray, None] = None
    model_config = ConfigDict(arbitrary_types_allowed=True)

    def to_dict(self, include_images=False):
        out = {"label": self.label, "detected": self.detected, "mode": self.mode}
        if include_images:
            out["aligned_image"] = self.aligned_image.tolist() if self.aligned_image is not None else None
            out["visualization_image"] = (self.visualization_image.tolist() if self.visualization_image is not None
                                          else None)
        out["boundary_bbox"] = self.boundary_bbox
        out["score"] = self.score
        return out


def _not_detected(mode: Optional[str]) -> DocumentBoundaryPrediction:
    return DocumentBoundaryPrediction(label="document", detected=False, mode=mode, aligned_image=None,
                                      visualization_image=None, boundary_bbox=[0, 0, 0, 0], score=0)


# ---------------------------------------------------------------------------------------------------- the plan
@dataclass
class RegistrationPlan:
    """What predict_document_image (unilm_dit.py:375-508) does with one page of ``width`` x ``height``: the chosen box, and
    the warp — crop window, resized size, where it lands on the canvas, the canvas, the marker centres and the returned
    size (a canvas of another shape is resized to it with INTER_CUBIC)."""
    detected: bool
    boundary_bbox: List[int] = field(default_factory=lambda: [0, 0, 0, 0])
    score: float = 0.0
    crop: Tuple[int, int, int, int] = (0, 0, 0, 0)          # x, y, w, h of the page window
    resized: Tuple[int, int] = (0, 0)                      # w, h
    offset: Tuple[int, int] = (0, 0)                       # left, top on the canvas
    canvas: Tuple[int, int] = (0, 0)                       # w, h
    markers: List[Tuple[int, int]] = field(default_factory=list)
    final: Tuple[int, int] = (0, 0)                        # w, h

    def desc(self) -> RegisterDesc:
        d = RegisterDesc()
        d.crop_x, d.crop_y, d.crop_w, d.crop_h = self.crop
        d.out_w, d.out_h = self.resized
        d.left, d.top = self.offset
        d.canvas_w, d.canvas_h = self.canvas
        d.n_markers = len(self.markers)
        for k, (x, y) in enumerate(self.markers):
            d.marker_x[k], d.marker_y[k] = x, y
        d.marker_radius = MARKER_RADIUS
        for c in range(3):
            d.marker_color[c] = MARKER_COLOR[c]
        d.final_w, d.final_h = self.final
        return d


def register_warp_host(ctx: Context, page: np.ndarray, plan: RegistrationPlan) -> np.ndarray:
    """The warp of a detected plan on a host page (HxWx3 uint8) -> the registered page (host)."""
    page = np.ascontiguousarray(page, np.uint8)
    fw, fh = plan.final
    out = np.empty((fh, fw, 3), np.uint8)
    d = plan.desc()
    check(ctx.h, ctx.lib.mhip_register_warp_host(ctx.h, page.ctypes.data_as(C.c_void_p), page.shape[0], page.shape[1],
                                                 C.byref(d), out.ctypes.data_as(C.c_void_p)), "mhip_register_warp_host")
    return out


def select_box(scores: Sequence[float]) -> Optional[int]:
    """unilm_dit.py:375-407.  One box is taken whatever its score; of several, the score filter (> 0.7) and a second
    class-aware NMS keep the best-scoring box when it clears the filter — the detections arrive score-ordered, so that is
    box 0 if scores[0] > 0.7, and nothing otherwise."""
    n = len(scores)
    if n == 0:
        return None
    if n == 1 or np.float32(scores[0]) > np.float32(MIN_SCORE):
        return 0
    return None


def _slice_len(start: int, length: int, size: int) -> int:
    """len(range(size)[start:start + length]) for start >= 0: numpy clips a slice at the edge"""
    return max(0, min(start + length, size) - min(start, size))


def registration_plan(width: int, height: int, boxes: np.ndarray, scores: np.ndarray, mode: Optional[str],
                      registration_point: Tuple[int, int] = (10, 10), margin_width: int = 5,
                      margin_height: int = 5) -> RegistrationPlan:
    """The registration of one ``width`` x ``height`` page from its detections (boxes xyxy page coordinates, score-ordered)."""
    W, H = int(width), int(height)
    i = select_box(scores)
    if i is None:
        return RegistrationPlan(detected=False)
    x0, y0, x1, y1 = (int(v) for v in np.asarray(boxes)[i])      # int(): truncation
    w, h = x1 - x0, y1 - y0
    p1_x, p1_y = (int(v) for v in registration_point)
    if p1_x < 0 or p1_y < 0:
        raise ValueError(f"registration point {registration_point} must not be negative")
    mw, mh = int(margin_width), int(margin_height)
    bbox = [max(0, x0 - mw), max(0, y0 - mh), min(W, w + mw * 2), min(H, h + mh * 2)]
    score = float(scores[i])
    crop_w, crop_h = _slice_len(bbox[0], bbox[2], W), _slice_len(bbox[1], bbox[3], H)
    crop = (min(bbox[0], W), min(bbox[1], H), crop_w, crop_h)
    if mode == "absolute":
        if p1_x + bbox[2] > W or p1_y + bbox[3] > H:
            return RegistrationPlan(detected=False)
        return RegistrationPlan(True, bbox, score, crop, (crop_w, crop_h), (p1_x, p1_y), (W, H), [(p1_x, p1_y)], (W, H))
    if mode == "fit_to_page":
        new_width = W - p1_x * 2
        out_w, out_h = crop_w, crop_h
        if bbox[3] > bbox[2]:
            r = new_width / float(crop_w)
            out_w, out_h = new_width, int(crop_h * r)
            if out_w <= 0 or out_h <= 0:
                raise ValueError(f"fit_to_page: cannot resize a {crop_w}x{crop_h} crop to {out_w}x{out_h}")
        bottom = max(0, int(H - out_h - p1_y))
        canvas = (out_w + 2 * p1_x, out_h + p1_y + bottom)
        return RegistrationPlan(True, bbox, score, crop, (out_w, out_h), (p1_x, p1_y), canvas,
                                [(p1_x, p1_y), (p1_x + new_width, p1_y)], (W, H))
    # any other mode: the white page the reference starts from
    return RegistrationPlan(True, bbox, score, (0, 0, 0, 0), (0, 0), (0, 0), (W, H), [], (W, H))


# ---------------------------------------------------------------------------------------------------- processors
def _frames_of(documents) -> Tuple[List[np.ndarray], bool]:
    """docarray-like documents (``.tensor`` / ``.tags``) or plain HxWx3 uint8 frames"""
    docs = len(documents) > 0 and hasattr(documents[0], "tensor")
    frames = [np.asarray(d.tensor if docs else d) for d in documents]
    return frames, docs


class BaseDocumentBoundaryRegistration:
    """marie/components/document_registration/base.py"""

    def predict(self, documents, registration_method: Optional[str], registration_point: Tuple[int, int],
                margin_width: int, margin_height: int, words: Optional[List[List[str]]] = None,
                boxes: Optional[List[List[List[int]]]] = None, batch_size: Optional[int] = None):
        raise NotImplementedError

    def run(self, documents, registration_method: str = "absolute", registration_point: Tuple[int, int] = (10, 10),
            margin_width: int = 5, margin_height: int = 5, words: Optional[List[List[str]]] = None,
            boxes: Optional[List[List[List[int]]]] = None, batch_size: Optional[int] = None):
        """Register ``documents``: objects with ``.tensor`` (the frame) and ``.tags`` get
        ``tags["document_boundary"]`` and are returned; a list of frames returns the list of predictions."""
        if registration_method not in ["absolute", "fit_to_page"]:
            raise ValueError(f"Invalid registration method: {registration_method}")
        if registration_point is None:
            raise ValueError("Registration point must be provided")
        if not isinstance(registration_point, tuple) or len(registration_point) != 2:
            raise ValueError("Registration point must be a tuple of two integers")
        if not documents:
            return []
        return self.predict(documents=documents, registration_method=registration_method,
                            registration_point=registration_point, margin_width=margin_width,
                            margin_height=margin_height, words=words, boxes=boxes, batch_size=batch_size)


class NoopDocumentBoundaryRegistration(BaseDocumentBoundaryRegistration):
    """unilm_dit.py:65-97: every document gets the not-detected prediction."""

    def __init__(self, **kwargs):
        pass

    def predict(self, documents, registration_method, registration_point, margin_width, margin_height, words=None,
                boxes=None, batch_size=None):
        preds = [_not_detected(registration_method) for _ in documents]
        _, docs = _frames_of(documents)
        if not docs:
            return preds
        for d, p in zip(documents, preds):
            d.tags["document_boundary"] = p
        return documents


class UnilmDocumentBoundaryRegistration(BaseDocumentBoundaryRegistration):
    """Drop-in for marie/components/document_registration/unilm_dit.py:100-531."""

    def __init__(self, model_name_or_path: Union[str, os.PathLike], model_version: Optional[str] = None,
                 use_gpu: bool = True, batch_size: int = 16, devices: Optional[List[Any]] = None,
                 show_error: Optional[Union[str, bool]] = True, debug_visualization: Optional[bool] = False, *,
                 state=None, precision: str = "f16", models_dir: Optional[str] = None, ctx: Optional[Context] = None):
        if not use_gpu:
            raise MarieHipError("UnilmDocumentBoundaryRegistration here is the MI355X path; use_gpu=False has no implementation")
        self.model_name_or_path = model_name_or_path      # logged, not used for the weights (as in the reference)
        self.show_error = show_error
        self.batch_size = int(batch_size)
        self.debug_visualization = True                   # forced, as unilm_dit.py:181: the shape restore always runs
        logger.info("Document registration : %s", model_name_or_path)
        if state is None:
            # MODEL.WEIGHTS of prod.yaml under the model zoo, looked up before a device context exists
            from .constants import __model_path__

            path = os.path.join(__model_path__ if models_dir is None else models_dir, MODEL_SUBPATH)
            if not os.path.exists(path):
                raise FileNotFoundError(f"File not found : {path}")
        prec = {"f16": PREC_F16, "fp16": PREC_F16, "f32": PREC_F32, "fp32": PREC_F32}[precision]
        self.ctx = ctx or Context(self._device_id(devices))
        if state is None:
            import torch

            sd = torch.load(path, map_location="cpu", weights_only=True)
            sd = sd.get("model", sd)
            state = {k: (v.numpy() if hasattr(v, "numpy") else np.asarray(v)) for k, v in sd.items()}
        self.model = DitModel(self.ctx, state, precision=prec, config=boundary_config(self.ctx.lib))
        self.min_size_test = [self.model.cfg.min_size_test, self.model.cfg.min_size_test]

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
        self.model.close()

    # -- detection + warp --------------------------------------------------------------------------------------------
    def _detect(self, page_devs, h: int, w: int):
        """detections of device pages of one size: [(boxes, scores, classes)]"""
        return self.model.detect_ex_device([d.data_ptr() for d in page_devs], h, w)

    def _warp(self, page_dev, plan: RegistrationPlan) -> np.ndarray:
        import torch

        h, w = page_dev.shape[:2]
        fw, fh = plan.final
        out = torch.empty((fh, fw, 3), dtype=torch.uint8, device=page_dev.device)
        cw, ch = plan.canvas
        scratch = (torch.empty((ch, cw, 3), dtype=torch.uint8, device=page_dev.device) if (cw, ch) != (fw, fh) else None)
        d = plan.desc()
        check(self.ctx.h, self.ctx.lib.mhip_register_warp(self.ctx.h, C.c_void_p(page_dev.data_ptr()), h, w, w * 3,
                                                          C.byref(d), C.c_void_p(scratch.data_ptr() if scratch is not None
                                                                                 else 0),
                                                          C.c_void_p(out.data_ptr())), "mhip_register_warp")
        return out.cpu().numpy()

    def _predict_frames(self, frames: List[np.ndarray], mode, registration_point, margin_width, margin_height,
                        batch_size: int) -> List[DocumentBoundaryPrediction]:
        import torch

        for f in frames:
            if f.ndim != 3 or f.shape[2] != 3:
                raise ValueError(f"expected HxWx3 frames, got {f.shape}")
        dev_name = f"cuda:{self.ctx.device_id}"
        self.ctx.set_stream(torch.cuda.current_stream(dev_name).cuda_stream)
        preds: List[Optional[DocumentBoundaryPrediction]] = [None] * len(frames)
        for s0 in range(0, len(frames), batch_size):
            idx = list(range(s0, min(s0 + batch_size, len(frames))))
            groups = {}
            for i in idx:
                groups.setdefault(frames[i].shape[:2], []).append(i)
            for (h, w), members in groups.items():
                devs = [torch.from_numpy(np.ascontiguousarray(frames[i], np.uint8)).to(dev_name) for i in members]
                dets = self._detect(devs, h, w)
                for i, dev, (boxes, scores, _classes) in zip(members, devs, dets):
                    plan = registration_plan(w, h, boxes, scores, mode, registration_point, margin_width, margin_height)
                    if not plan.detected:
                        preds[i] = _not_detected(mode)
                        continue
                    preds[i] = DocumentBoundaryPrediction(label="document", detected=True, mode=mode,
                                                          aligned_image=self._warp(dev, plan), visualization_image=None,
                                                          boundary_bbox=plan.boundary_bbox, score=plan.score)
        return preds

    def predict(self, documents, registration_method: Optional[str], registration_point: Tuple[int, int],
                margin_width: int, margin_height: int, words: Optional[List[List[str]]] = None,
                boxes: Optional[List[List[List[int]]]] = None, batch_size: Optional[int] = None):
        """unilm_dit.py:207-273 (``words`` / ``boxes`` are accepted and unused, as there)."""
        if len(documents) == 0:
            return documents
        frames, docs = _frames_of(documents)
        preds = self._predict_frames(frames, registration_method, registration_point, margin_width, margin_height,
                                     int(batch_size or self.batch_size))
        if not docs:
            return preds
        for d, p in zip(documents, preds):
            d.tags["document_boundary"] = p
        return documents

    def predict_document_image(self, image: np.ndarray, registration_mode: str, registration_point: Tuple[int, int],
                               margin_width: int, margin_height: int, words=None, boxes=None, top_k: int = 1,
                               doc_id: Optional[str] = None) -> List[DocumentBoundaryPrediction]:
        """unilm_dit.py:275-531 for one frame: a one-element list."""
        return self._predict_frames([np.asarray(image)], registration_mode, registration_point, margin_width,
                                    margin_height, 1)
