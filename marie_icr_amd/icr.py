"""Production ICR recognizer (TPS-ResNet-BiLSTM-Attn) on MI355X behind the reference's ``CraftOcrProcessor`` surface.

Mirrors ``CraftOcrProcessor`` (reference: marie/document/craft_ocr_processor.py:26-286): same constructor arguments
(``work_dir, models_dir, cuda``), the checkpoint path ``<models_dir>/TPS-ResNet-BiLSTM-Attn-case-sensitive-ft/
best_accuracy.pth`` (:39-43), ``is_available()`` and ``recognize_from_fragments(images)``.  Crop batching
(Pillow-exact, img_w = 100), TPS rectification, ResNet-45, BiLSTM and the 49-step attention decoder run in
libmarie_hip.so; this file applies the reference's "[s]" cut / confidence rule to the per-step arg-max and softmax-max.

Deviation: a line whose decoded string starts with "[s]" yields ``{"text": "", "confidence": 0}`` for THAT line only; the
reference raises inside its batch loop there and drops the remaining lines of the batch (:253-285).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from ._lib import PREC_F16, PREC_F32, STAGE_GUARD, Context, MarieHipError, ModelHandle, check
from .crnn import IMG_H, pack_fragments
from .ocr_processor import OcrProcessor
from .weights import CRNN_CHARSET, ICR_IMG_W


class IcrModel(ModelHandle):
    """Device-resident TPS-ResNet-BiLSTM-Attn weights + forward.  Thin handle over ``mhip_icr``."""

    def __init__(self, ctx: Context, state: Optional[Dict[str, np.ndarray]], num_class: int = 96,
                 precision: int = PREC_F16):
        self.num_class = int(num_class)
        self.precision = int(precision)
        self.steps = ctx.lib.mhip_icr_steps()
        super().__init__(ctx, "icr", self.precision, self.num_class)
        if state is not None:
            self.load_state(state)

    def forward_host(self, crops_u8: np.ndarray, want_logits: bool = False, want_rectified: bool = False):
        """crops_u8: (n, 32, 100) uint8.  Returns dict of host arrays: argmax (n,49), pmax (n,49) [, logits, rectified]."""
        crops = np.ascontiguousarray(crops_u8, dtype=np.uint8)
        if crops.ndim != 3 or crops.shape[1:] != (IMG_H, ICR_IMG_W):
            raise ValueError(f"crops must be (n, {IMG_H}, {ICR_IMG_W}) uint8, got {crops.shape}")
        n = crops.shape[0]
        s = self.steps
        logits = np.empty((n, s, self.num_class), np.float32) if want_logits else None
        rect = np.empty((n, IMG_H, ICR_IMG_W), np.float32) if want_rectified else None
        argmax = np.empty((n, s), np.int32)
        pmax = np.empty((n, s), np.float32)
        if n:
            vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)  # noqa: E731
            check(self.ctx.h, self.lib.mhip_icr_forward_host(self.h, vp(crops), n, vp(logits), vp(argmax), vp(pmax),
                                                             vp(rect)), "mhip_icr_forward_host")
        return {"logits": logits, "argmax": argmax, "pmax": pmax, "rectified": rect}


def attn_texts(argmax: np.ndarray, pmax: np.ndarray, charset: str):
    """The reference's decode + "[s]" cut + confidence (marie/document/craft_ocr_processor.py:244-272,
    AttnLabelConverter.decode marie/models/icr/utils.py:142-148): the cut position is found in the joined STRING and the
    same number is used to slice the per-step probabilities."""
    character = ["[GO]", "[s]"] + list(charset)
    texts: List[str] = []
    confs: List[float] = []
    for row, pm in zip(argmax.tolist(), pmax):
        pred = "".join(character[i] for i in row)
        eos = pred.find("[s]")
        pred, pm = pred[:eos], pm[:eos]
        if pm.size == 0:
            texts.append("")
            confs.append(0.0)
        else:
            conf = np.float32(1.0)
            for v in pm:                       # cumprod in fp32, left to right
                conf = np.float32(conf * v)
            texts.append(pred.upper())
            confs.append(float(conf))
    return texts, confs


# ---------------------------------------------------------------------------------------------------------------------------
# Stage entries of csrc/icr_ops.hip (include/marie_hip.h): one kernel each on host arrays through the launcher the model
# calls.  Activations are fp32 here (narrowed to f16 and widened again in the f16 mode).  Every returned array is FLAT and
# STAGE_GUARD elements longer than the output proper: the tail comes back as the 0xff fill the device buffer got before the
# launch unless the kernel wrote past its end.
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _guarded(n: int, dtype=np.float32) -> np.ndarray:
    return np.zeros(int(n) + STAGE_GUARD, dtype)


def conv_gray_first(ctx: Context, precision: int, img: np.ndarray, w9xC, scale, bias) -> np.ndarray:
    """img (B, H, W) uint8 or fp32; w9xC (9, C) -> (B*H*W*64 + guard,)"""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8:
        img = _f32(img)
    B, H, W = img.shape
    w9xC, scale, bias = _f32(w9xC), _f32(scale), _f32(bias)
    out = _guarded(B * H * W * 64)
    check(ctx.h, ctx.lib.mhip_conv_gray_first_host(ctx.h, int(precision), int(img.dtype == np.uint8), _vp(img), B, H, W,
                                                   w9xC.shape[1], _vp(w9xC), _vp(scale), _vp(bias), _vp(out)),
          "mhip_conv_gray_first_host")
    return out


def maxpool_s21_p01(ctx: Context, precision: int, x: np.ndarray) -> np.ndarray:
    """x (B, H, W, C) -> (B*(H//2)*(W+1)*C + guard,)"""
    x = _f32(x)
    B, H, W, Cn = x.shape
    out = _guarded(B * (H // 2) * (W + 1) * Cn)
    check(ctx.h, ctx.lib.mhip_maxpool_s21_p01_host(ctx.h, int(precision), _vp(x), B, H, W, Cn, _vp(out)),
          "mhip_maxpool_s21_p01_host")
    return out


def avgpool_hw(ctx: Context, precision: int, x: np.ndarray) -> np.ndarray:
    """x (B, HW, C) -> (B*C + guard,)"""
    x = _f32(x)
    B, HW, Cn = x.shape
    out = _guarded(B * Cn)
    check(ctx.h, ctx.lib.mhip_avgpool_hw_host(ctx.h, int(precision), _vp(x), B, HW, Cn, _vp(out)), "mhip_avgpool_hw_host")
    return out


def tps_sample(ctx: Context, crops_u8: np.ndarray, c_prime, inv_delta_c, p_hat) -> np.ndarray:
    """crops (B, H, W) uint8, c_prime (B, F, 2), inv_delta_c (F+3, F+3), p_hat (H*W, F+3) -> (B*H*W + guard,)"""
    crops = np.ascontiguousarray(crops_u8, dtype=np.uint8)
    B, H, W = crops.shape
    c_prime, inv_delta_c, p_hat = _f32(c_prime), _f32(inv_delta_c), _f32(p_hat)
    F = c_prime.shape[1]
    if c_prime.shape != (B, F, 2) or inv_delta_c.shape != (F + 3, F + 3) or p_hat.shape != (H * W, F + 3):
        raise ValueError("tps_sample: shapes disagree")
    out = _guarded(B * H * W)
    check(ctx.h, ctx.lib.mhip_tps_sample_host(ctx.h, _vp(crops), _vp(c_prime), _vp(inv_delta_c), _vp(p_hat), B, H, W, F,
                                              _vp(out)), "mhip_tps_sample_host")
    return out


def attn_context(ctx: Context, precision: int, hproj, hp, score_w, H) -> np.ndarray:
    """hproj (B, T, 256), hp (B, ld_hp), score_w (256,), H (B, T, 256) -> (B*256 + guard,)"""
    hproj, hp, score_w, H = _f32(hproj), _f32(hp), _f32(score_w), _f32(H)
    B, T = H.shape[:2]
    if hproj.shape != (B, T, 256) or H.shape != (B, T, 256) or hp.shape[0] != B or score_w.shape != (256,):
        raise ValueError("attn_context: shapes disagree")
    out = _guarded(B * 256)
    check(ctx.h, ctx.lib.mhip_attn_context_host(ctx.h, int(precision), _vp(hproj), _vp(hp), hp.shape[1], _vp(score_w), _vp(H),
                                                B, T, _vp(out)), "mhip_attn_context_host")
    return out


def attn_cell(ctx: Context, precision: int, gctx, ghid, w_onehot, chars, c_prev):
    """gctx (B, 1024), ghid (B, ld_hp), w_onehot (num_class, 1024), chars (B,) int32, c_prev (B, 256) ->
    (c (B*256 + guard,), h (B*256 + guard,))"""
    gctx, ghid, w_onehot = _f32(gctx), _f32(ghid), _f32(w_onehot)
    chars = np.ascontiguousarray(chars, dtype=np.int32)
    B = gctx.shape[0]
    if gctx.shape != (B, 1024) or ghid.shape[0] != B or w_onehot.shape[1] != 1024 or chars.shape != (B,):
        raise ValueError("attn_cell: shapes disagree")
    c = _guarded(B * 256)
    c[:B * 256] = _f32(c_prev).reshape(-1)
    h = _guarded(B * 256)
    check(ctx.h, ctx.lib.mhip_attn_cell_host(ctx.h, int(precision), _vp(gctx), _vp(ghid), ghid.shape[1], _vp(w_onehot),
                                             w_onehot.shape[0], _vp(chars), B, _vp(c), _vp(h)), "mhip_attn_cell_host")
    return c, h


def argmax_rows(ctx: Context, logits: np.ndarray, C_used: int) -> np.ndarray:
    """logits (B, ld) fp32, the first C_used columns count -> (B + guard,) int32"""
    logits = _f32(logits)
    B, ld = logits.shape
    idx = _guarded(B, np.int32)
    check(ctx.h, ctx.lib.mhip_argmax_rows_host(ctx.h, _vp(logits), ld, int(C_used), B, _vp(idx)), "mhip_argmax_rows_host")
    return idx


def rowmax_softmax(ctx: Context, logits: np.ndarray):
    """logits (rows, C) fp32 -> (idx (rows + guard,) int32, pmax (rows + guard,) fp32)"""
    logits = _f32(logits)
    rows, Cn = logits.shape
    idx, pmax = _guarded(rows, np.int32), _guarded(rows)
    check(ctx.h, ctx.lib.mhip_rowmax_softmax_host(ctx.h, _vp(logits), rows, Cn, _vp(idx), _vp(pmax)),
          "mhip_rowmax_softmax_host")
    return idx, pmax


class CraftOcrProcessor(OcrProcessor):
    """Drop-in for marie/document/craft_ocr_processor.py:26."""

    def __init__(self, work_dir: str = "/tmp/icr", models_dir: Optional[str] = None, cuda: bool = True, *,
                 state: Optional[Dict[str, np.ndarray]] = None, character: str = CRNN_CHARSET, precision: str = "f16",
                 device_id: int = 0, ctx: Optional[Context] = None, **kwargs) -> None:
        super().__init__(work_dir, cuda)
        if not cuda:
            raise MarieHipError("CraftOcrProcessor here is the MI355X path; cuda=False has no implementation")
        self.character = character
        if state is None:
            # craft_ocr_processor.py:30,38-42: models_dir defaults to <model zoo>/icr; looked up before a device context exists
            from .constants import __model_path__

            models_dir = os.path.join(__model_path__, "icr") if models_dir is None else models_dir
            path = os.path.join(models_dir, "TPS-ResNet-BiLSTM-Attn-case-sensitive-ft", "best_accuracy.pth")
            if not os.path.exists(path):
                raise FileNotFoundError(f"File not found : {path}")
        self.ctx = ctx or Context(device_id)
        self.batch_size = int(kwargs.get("batch_size", 2048))
        if state is None:
            import torch

            sd = torch.load(path, map_location="cpu", weights_only=True)
            state = {k: v.numpy() for k, v in sd.items()}
        prec = {"f16": PREC_F16, "fp16": PREC_F16, "f32": PREC_F32, "fp32": PREC_F32}[precision]
        self.model = IcrModel(self.ctx, state, num_class=len(character) + 2, precision=prec)

    def is_available(self) -> bool:
        return self.model is not None

    def _crops(self, images: Sequence[np.ndarray]) -> np.ndarray:
        """GPU crop batcher (Pillow-exact bicubic to 32 x 100 + replicate pad) -> host uint8 (n, 32, 100)."""
        import torch

        packed, descs = pack_fragments(images)
        d_in = torch.from_numpy(packed).cuda()
        d_out = torch.empty((len(images), IMG_H, ICR_IMG_W), dtype=torch.uint8, device="cuda")
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        check(self.ctx.h, self.ctx.lib.mhip_crop_batch(self.ctx.h, C.c_void_p(d_in.data_ptr()), descs, len(images),
                                                       ICR_IMG_W, C.c_void_p(d_out.data_ptr())), "mhip_crop_batch")
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    def recognize_from_fragments(self, images, **kwargs) -> List[Dict[str, object]]:
        results: List[Dict[str, object]] = []
        for start in range(0, len(images), self.batch_size):
            batch = images[start:start + self.batch_size]
            out = self.model.forward_host(self._crops(batch))
            texts, confs = attn_texts(out["argmax"], out["pmax"], self.character)
            for k, (text, conf) in enumerate(zip(texts, confs)):
                results.append({"confidence": conf, "text": text, "id": f"img-{start + k}"})
        return results
