"""Writes tests/golden/indexer.json: the reference document indexer's own post-model procedure on seeded cases.

usage: python tools/gen_indexer_golden.py <root of the reference checkout> [out.json]

The reference file (marie/components/document_indexer/transformers.py) and the helpers it calls (marie/utils/overlap.py,
marie/boxes/line_processor.py) are loaded by path and run as they are; everything else they import (``marie.*`` plumbing,
``docarray``, the ``transformers`` classes, the drawing helpers) is a stand-in module built here.  The indexer object is made
without its constructor; its ``processor`` hands back the windows this project's tokeniser cut and its ``model`` the logits
of the case, so ``inference`` runs from the logits on, then ``postprocess`` with an engine that answers every region with a
fixed text.  Not run by any test (the reference checkout does not travel with this repository); it writes images under
/tmp/tensors, as the reference does.
"""
from __future__ import annotations

import enum
import importlib.util
import json
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference(ref_root: str):
    """the reference's TransformersDocumentIndexer class under stand-in modules"""
    marie = os.path.join(ref_root, "marie")

    class _Any:
        def __init__(self, *a, **k):
            pass

        def __class_getitem__(cls, item):
            return cls

    class PSMode(enum.Enum):
        RAW_LINE = "raw_line"

    class CoordinateFormat(enum.Enum):
        XYWH = "xywh"

    class MarieLogger:
        def __init__(self, name):
            self.logger = logging.getLogger(name)

    if importlib.util.find_spec("cv2") is None:
        _module("cv2")
    _module("docarray", DocList=_Any)
    _module("transformers", AutoModelForTokenClassification=_Any, LayoutLMv3FeatureExtractor=_Any, LayoutLMv3Processor=_Any,
            LayoutLMv3TokenizerFast=_Any)
    for pkg in ("marie", "marie.components", "marie.components.document_indexer", "marie.executor", "marie.executor.ner",
                "marie.logging_core", "marie.models", "marie.utils", "marie.api", "marie.boxes", "marie.ocr", "marie.registry"):
        _module(pkg)
    sys.modules["marie.boxes"].PSMode = PSMode
    sys.modules["marie.ocr"].CoordinateFormat = CoordinateFormat
    sys.modules["marie.ocr"].OcrEngine = _Any
    _module("marie.constants", __marie_home__="/tmp/marie", __model_path__="/tmp/marie/model_zoo")
    _module("marie.logging_core.logger", MarieLogger=MarieLogger)
    _module("marie.logging_core.predefined", default_logger=logging.getLogger("marie"))
    _module("marie.logging_core.profile", TimeContext=_Any)
    _module("marie.models.utils", initialize_device_settings=lambda **k: ([], 0))
    _module("marie.api.docs", BatchableMarieDoc=_Any, MarieDoc=_Any)
    _module("marie.ocr.ocr_engine", reset_bbox_cache=lambda: None)
    _module("marie.ocr.util", get_known_ocr_engines=lambda **k: {})
    _module("marie.registry.model_registry", ModelRegistry=_Any)
    _module("marie.utils.docs", convert_frames=lambda frames, **k: frames, frames_from_docs=lambda docs: docs)
    _module("marie.utils.image_utils", hash_frames_fast=lambda frames: "golden")
    _module("marie.utils.json", load_json_file=None, store_json_object=lambda *a, **k: None)
    _module("marie.utils.utils", ensure_exists=lambda p: os.makedirs(p, exist_ok=True))
    _module("marie.components.document_indexer.base", BaseDocumentIndexer=_Any)
    _module("marie.components.document_indexer.validator", AddressValidator=_Any)
    _load("marie.utils.overlap", os.path.join(marie, "utils", "overlap.py"))
    _load("marie.boxes.line_processor", os.path.join(marie, "boxes", "line_processor.py"))
    real = _load("marie.executor.ner.utils_real", os.path.join(marie, "executor", "ner", "utils.py"))
    _module("marie.executor.ner.utils", draw_box=lambda *a, **k: None, get_font=lambda size: None,
            get_random_color=lambda: (0, 0, 0, 70), normalize_bbox=real.normalize_bbox, unnormalize_box=real.unnormalize_box,
            visualize_extract_kv=lambda *a, **k: None, visualize_prediction=lambda *a, **k: None)
    mod = _load("marie.components.document_indexer.transformers",
                os.path.join(marie, "components", "document_indexer", "transformers.py"))
    return mod.TransformersDocumentIndexer


class StubEngine:
    """answers every region with a text made of its id; records what it was asked"""

    def __init__(self):
        self.calls = []

    def extract(self, frames, pms_mode, coordinate_format, regions, **kwargs):
        self.calls.append([dict(r) for r in regions])
        return {"regions": [{"id": r["id"], "text": f"text of {r['id']}", "confidence": 0.5 + 0.01 * (k % 40)}
                            for k, r in enumerate(regions)]}


def run_reference(cls, case, marie_json):
    """one case through the reference's inference (from the logits on) and postprocess"""
    import torch
    from PIL import Image

    import indexer_cases as IC

    enc = IC.case_arrays(case)
    n = enc["logits"].shape[0]

    class Encoding(dict):
        @property
        def bbox(self):
            return self["bbox"]

    def processor(image, words, boxes=None, **kwargs):
        offs = np.zeros((n, 512, 2), np.int64)
        offs[..., 0] = np.where(enc["first"], 0, 1)
        offs[..., 1] = offs[..., 0] + 1
        return Encoding(input_ids=torch.zeros((n, 512), dtype=torch.long), attention_mask=torch.ones((n, 512), dtype=torch.long),
                        bbox=torch.from_numpy(enc["bbox"].astype(np.int64)), pixel_values=[torch.zeros((3, 224, 224))] * n,
                        offset_mapping=torch.from_numpy(offs), overflow_to_sample_mapping=torch.zeros((n,), dtype=torch.long))

    class Out:
        logits = torch.from_numpy(enc["logits"])

    obj = object.__new__(cls)
    obj.logger = logging.getLogger("indexer")
    obj.model = lambda **kw: Out
    obj.processor = processor
    obj.device = torch.device("cpu")
    obj.init_configuration = marie_json
    obj.labels = marie_json["labels"]
    obj.debug_visuals = obj.debug_visuals_overlay = obj.debug_visuals_ner = False
    obj.ocr_engine = StubEngine()
    os.makedirs("/tmp/tensors", exist_ok=True)
    frame = Image.fromarray(np.full((case["height"], case["width"], 3), 255, np.uint8))
    pred, boxes, scores = obj.inference(frame, case["words"], case["boxes_norm"], marie_json["labels"], 0.5)
    annotation = {"meta": {"imageSize": {"width": case["width"], "height": case["height"]}, "page": 0}, "predictions": pred,
                  "boxes": boxes, "scores": scores}
    results = obj.postprocess([frame], [annotation], [case["words"]], [case["boxes"]], "golden")
    return {"inference": [pred, boxes, scores], "results": results, "regions": obj.ocr_engine.calls}


def _plain(o):
    if isinstance(o, np.generic):
        return o.item()
    if isinstance(o, np.ndarray):
        return o.tolist()
    if hasattr(o, "__dict__"):
        return o.__dict__
    raise TypeError(type(o))


def main():
    import indexer_cases as IC

    ref_root = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "indexer.json")
    cls = load_reference(ref_root)
    marie_json = IC.marie_config()
    golden = {"marie": marie_json, "cases": []}
    for case in IC.make_cases():
        want = json.loads(json.dumps(run_reference(cls, case, marie_json), default=_plain))
        golden["cases"].append({"name": case["name"], "expected": want})
        print(case["name"], "windows", len(case["windows"]), "kv", len(want["results"]["kv"]), "ner", len(want["results"]["ner"]),
              "groups", len(want["results"]["groups"]))
    with open(out, "w", encoding="utf-8") as f:
        json.dump(golden, f, separators=(",", ":"))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
