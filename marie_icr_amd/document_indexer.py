"""The document indexer (named-entity recognition) that runs directly on the OCR result: LayoutLMv3 token classification over
the page image, the OCR words and their boxes, then the grouping of the word tags into key/value pairs, NER fields and composite
entities, and a second read of the found regions through the OCR engine.

reference: ``TransformersDocumentIndexer`` (marie/components/document_indexer/transformers.py:91-1243), ``normalize_bbox`` /
``unnormalize_box`` (marie/executor/ner/utils.py:13-28), ``find_overlap_horizontal`` (marie/utils/overlap.py:106-183) and, for
what the reference delegates to the transformers library, ``LayoutLMv3Processor`` with ``LayoutLMv3TokenizerFast`` (words + boxes
-> windows of 512 tokens that overlap by 128, with offsets) and ``LayoutLMv3ForTokenClassification``.

The model runs in HIP (``layoutlmv3.py``): per token it returns the arg-max label and its soft-max probability, nothing else
crosses to the host.  All windows of all pages of a batch go through one model call, and the windows of a page share the page's
resize and patch projection (the reference loops page by page and hands the model one copy of the page per window).  Everything
after the model call is host logic in the reference too; it is restated here step by step, its quirks included.
There is no CPU path: ``use_gpu=False`` raises.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import PREC_F16, PREC_F32, Context, MarieHipError
from .box_processor import PSMode, find_line_number
from .document_classifier import MAX_LENGTH, ByteLevelBPE, _load_state
from .geometry import line_merge
from .ocr_processor import merge_bboxes_as_block

STRIDE = 128              # inference: stride=128, max_length=512


def unnormalize_box(bbox, width, height):
    """marie/executor/ner/utils.py:13-19."""
    return [width * (bbox[0] / 1000), height * (bbox[1] / 1000), width * (bbox[2] / 1000), height * (bbox[3] / 1000)]


def normalize_bbox(bbox, size):
    """marie/executor/ner/utils.py:22-28."""
    return [int(1000 * bbox[0] / size[0]), int(1000 * bbox[1] / size[1]), int(1000 * bbox[2] / size[0]),
            int(1000 * bbox[3] / size[1])]


def find_overlap_horizontal(box, bboxes, center_y_overlap=None):
    """1-D horizontal IoU of ``box`` (x, y, w, h) against every box of ``bboxes``; identical boxes are skipped.
    reference: marie/utils/overlap.py:106-183."""
    overlaps, indexes, scores = [], [], []
    if len(bboxes) == 0:
        return [], [], []
    x, y, w, h = box
    x1min, x1max = x, x + w
    center_start = center_end = 0
    if center_y_overlap is not None:
        center_start = (y + h // 2) - (h * center_y_overlap)
        center_end = (y + h // 2) + (h * center_y_overlap)
    for i, bb in enumerate(bboxes):
        _x, _y, _w, _h = bb
        x2min, x2max = _x, _x + _w
        if box[0] == bb[0] and box[1] == bb[1] and box[2] == bb[2] and box[3] == bb[3]:
            continue
        if x1min < x2max and x2min < x1max:
            if center_y_overlap is not None and (_y + _h // 2 < center_start or _y + _h // 2 > center_end):
                continue
            inter = min(x1max, x2max) - max(x1min, x2min)
            iou = max(min(inter / float(w + _w - inter), 1.0), 0.0)
            scores.append(iou)
            overlaps.append(bb)
            indexes.append(i)
    return overlaps, indexes, scores


@dataclass
class LineGroup:
    bbox: list
    key: str
    line: int
    score: float


@dataclass
class EntityGroup:
    bbox: list
    key: str
    group: List[LineGroup]
    components: List[str]


def merge_window_predictions(labels: Sequence[str], win_labels, win_scores, win_bbox, win_first, width: int, height: int):
    """transformers.py:576-654: the per-window filtering and the merge of overlapping windows, from the model's decision on.
    ``win_labels`` / ``win_scores`` [n_win][T]: arg-max index and its soft-max probability per token; ``win_bbox`` [n_win][T][4]
    the token boxes on the 0..1000 grid; ``win_first`` [n_win][T]: ``offset_mapping[:, 0] == 0``.
    -> (predictions, boxes in pixels, scores) per kept token.

    Restated with its quirks: special and padding tokens count as "not a sub-word" and leave by their [0, 0, 0, 0] box; the
    score list is filtered against the already filtered box list, so it keeps its first ``len(boxes)`` entries (every kept token
    carries the score of the kept token before it, the first one ``<s>``'s); the duplicate-box loop pops while it iterates; a
    later window's prediction replaces an earlier one for the same box only when its score is ``>=``."""
    out_prediction: List[str] = []
    out_boxes: List[List[int]] = []
    out_scores: List[float] = []
    for batch_index in range(len(win_labels)):
        predictions = [int(v) for v in win_labels[batch_index]]
        token_boxes = [[int(c) for c in b] for b in win_bbox[batch_index]]
        probabilities = [float(v) for v in win_scores[batch_index]]
        is_subword = [not bool(f) for f in win_first[batch_index]]
        true_predictions = [labels[pred] for idx, pred in enumerate(predictions) if not is_subword[idx]]
        true_boxes = [unnormalize_box(box, width, height) for idx, box in enumerate(token_boxes) if not is_subword[idx]]
        true_boxes = [[int(b) for b in box] for box in true_boxes]
        true_scores = [round(probabilities[idx], 6) for idx, val in enumerate(predictions) if not is_subword[idx]]
        assert len(true_predictions) == len(true_boxes) == len(true_scores)
        true_predictions = [pred for pred, box in zip(true_predictions, true_boxes) if box != [0, 0, 0, 0]]
        true_boxes = [box for box in true_boxes if box != [0, 0, 0, 0]]
        true_scores = [score for score, box in zip(true_scores, true_boxes) if box != [0, 0, 0, 0]]
        for box in true_boxes:
            if true_boxes.count(box) > 1:
                current_idx = true_boxes.index(box)
                true_predictions.pop(current_idx)
                true_boxes.pop(current_idx)
                true_scores.pop(current_idx)
        if batch_index > 0:
            for idx, box in enumerate(out_boxes):
                if box in true_boxes:
                    current_idx = true_boxes.index(box)
                    if true_scores[current_idx] >= out_scores[idx]:
                        out_prediction[idx] = true_predictions[current_idx]
                        out_scores[idx] = true_scores[current_idx]
                    true_predictions.pop(current_idx)
                    true_boxes.pop(current_idx)
                    true_scores.pop(current_idx)
        out_prediction.extend(true_predictions)
        out_boxes.extend(true_boxes)
        out_scores.extend(true_scores)
    return out_prediction, out_boxes, out_scores


class TransformersDocumentIndexer:
    """marie/components/document_indexer/transformers.py:91-1243.

    ``model_name_or_path`` is a local directory with ``marie.json``, ``config.json``, the weights (``pytorch_model.bin`` or
    ``model.safetensors``) and, unless ``tokenizer`` names another directory, ``vocab.json`` + ``merges.txt``.  ``state`` /
    ``config`` / ``init_configuration`` (a state dict under the Hugging Face key names, a ``config.json`` dictionary, the
    ``marie.json`` dictionary) replace the files of the same content."""

    def __init__(self, model_name_or_path: str, model_version: Optional[str] = None, tokenizer: Optional[str] = None,
                 use_gpu: bool = True, top_k: Optional[int] = 1, task: str = "transformers-document-indexer",
                 batch_size: int = 16, use_auth_token=None, devices=None, show_error=True, ocr_engine=None, *,
                 state: Optional[Dict[str, np.ndarray]] = None, config: Optional[dict] = None,
                 init_configuration: Optional[dict] = None, precision: str = "f16", ctx: Optional[Context] = None, **kwargs):
        if task != "transformers-document-indexer":
            raise ValueError(f"Unsupported task: {task}")
        if not use_gpu:
            raise MarieHipError("TransformersDocumentIndexer runs on the GPU only: there is no CPU path in this project")
        if precision not in ("f16", "f32"):
            raise ValueError(f"precision {precision!r}: 'f16' or 'f32'")
        if not os.path.isdir(model_name_or_path):
            raise FileNotFoundError(f"model directory {model_name_or_path!r} does not exist (models are local directories)")
        self.show_error, self.batch_size, self.task, self.top_k = show_error, int(batch_size), task, top_k
        self.model_dir = model_name_or_path
        if init_configuration is None:
            config_path = os.path.join(model_name_or_path, "marie.json")
            if not os.path.exists(config_path):
                raise FileNotFoundError("Expected config 'marie.json' not found in model directory")
            with open(config_path, encoding="utf-8") as f:
                init_configuration = json.load(f)
        self.init_configuration = init_configuration
        self.debug_scores = bool(init_configuration.get("debug", {}).get("scores", False))
        self.labels = list(init_configuration["labels"])
        tok_dir = tokenizer if tokenizer is not None else model_name_or_path
        self.tokenizer = ByteLevelBPE(os.path.join(tok_dir, "vocab.json"), os.path.join(tok_dir, "merges.txt"))
        if config is None:
            with open(os.path.join(model_name_or_path, "config.json"), encoding="utf-8") as f:
                config = json.load(f)
        self.hf_config = dict(config)
        self.precision = PREC_F16 if precision == "f16" else PREC_F32
        self.ocr_engine = ocr_engine
        self._open_model(state, ctx)

    def _open_model(self, state, ctx):
        from .layoutlmv3 import LayoutLMv3Model, config_from_hf

        self.ctx = ctx if ctx is not None else Context(0)
        cfg = config_from_hf(self.hf_config, self.ctx.lib)
        cfg.num_labels = len(self.labels)              # __load_model: num_labels=len(labels)
        most = self.ctx.lib.mhip_layoutlmv3_max_token_labels(cfg.hidden)
        if cfg.num_labels > most:
            raise MarieHipError(f"num_labels {cfg.num_labels} beyond the {most} the token head covers at hidden {cfg.hidden}")
        if cfg.pad_id != self.tokenizer.pad_id:
            raise ValueError(f"config.json pad_token_id {cfg.pad_id} differs from the tokeniser's <pad> id {self.tokenizer.pad_id}")
        if state is None:
            state = _load_state(self.model_dir)
        self.model = LayoutLMv3Model(self.ctx, state, cfg, self.precision)

    def _tag(self, pages: List[np.ndarray], window_page: np.ndarray, ids: np.ndarray, bbox: np.ndarray, mask: np.ndarray):
        """One model call over all windows -> (labels (n_win, 512) int, scores (n_win, 512) fp32)."""
        import torch

        from .layoutlmv3 import pack_pages

        packed, descs = pack_pages(pages)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        d_in = torch.from_numpy(packed).cuda()
        out = self.model.tag_device(d_in.data_ptr(), descs, len(pages), window_page, ids, bbox, mask)   # returns after the stream drained
        return out["labels"], out["scores"]

    def get_label_info(self, labels: List[str]):
        id2label = {v: k for v, k in enumerate(labels)}
        label2id = {k: v for v, k in enumerate(labels)}
        return labels, id2label, label2id

    @staticmethod
    def _frame(image) -> np.ndarray:
        a = np.asarray(image)
        if a.ndim == 2:
            a = np.repeat(a[:, :, None], 3, axis=2)
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"page image must be H x W x 3 uint8, got {a.shape} {a.dtype}")
        return np.ascontiguousarray(a)

    def preprocess(self, frames: List, words: List[List[str]], boxes: List[List[List[int]]]):
        """transformers.py:277-300: frames as H x W x 3 arrays, the boxes (x, y, w, h) scaled to the 0..1000 grid."""
        assert len(frames) == len(boxes) == len(words)
        frames = [self._frame(f) for f in frames]
        normalized_boxes = []
        for frame, box_set in zip(frames, boxes):
            size = (frame.shape[1], frame.shape[0])
            normalized_boxes.append([normalize_bbox(box, size) for box in box_set])
        assert len(frames) == len(normalized_boxes) == len(words)
        return frames, words, normalized_boxes

    def _encode(self, words, boxes):
        for b in boxes:
            if min(b) < 0 or max(b) > 1000:
                raise IndexError("The `bbox` coordinate values should be within 0-1000 range.")
        return self.tokenizer.encode_windows([str(w) for w in words], boxes, MAX_LENGTH, STRIDE)

    def _inference_pages(self, frames: List[np.ndarray], words, boxes, labels: List[str]):
        """``inference`` of several pages through one model call -> [(predictions, boxes, scores)] per page."""
        enc = [self._encode(w, b) for w, b in zip(words, boxes)]
        window_page = np.concatenate([np.full((e[0].shape[0],), k, np.int32) for k, e in enumerate(enc)])
        ids, bbox, mask = (np.concatenate([e[j] for e in enc]) for j in range(3))
        win_labels, win_scores = self._tag(frames, window_page, ids, bbox, mask)
        out, at = [], 0
        for frame, w, b, e in zip(frames, words, boxes, enc):
            n = e[0].shape[0]
            height, width = frame.shape[:2]
            pred, pbox, score = merge_window_predictions(labels, win_labels[at:at + n], win_scores[at:at + n], e[1], e[3], width, height)
            at += n
            original_boxes = [[int(v) for v in unnormalize_box(box, width, height)] for box in b]
            pred, pbox, score = self.align_predictions(w, original_boxes, pred, pbox, score)
            assert len(pred) == len(w) == len(b)
            out.append((pred, pbox, score))
        return out

    def inference(self, image: Any, words: List[Any], boxes: List[Any], labels: List[str], threshold: float):
        """transformers.py:481-666: boxes normalised to 1000 -> (predictions, boxes in pixels, scores) per word."""
        assert len(words) == len(boxes)
        return self._inference_pages([self._frame(image)], [words], [boxes], labels)[0]

    def align_predictions(self, words, original_boxes, out_prediction, out_boxes, out_scores):
        """transformers.py:668-701: the prediction of every word, found by the equality of its box."""
        aligned_prediction, aligned_boxes, aligned_scores = [], [], []
        for idx, word in enumerate(words):
            box = original_boxes[idx]
            if box in out_boxes:
                current_idx = out_boxes.index(box)
                aligned_prediction.append(out_prediction[current_idx])
                aligned_boxes.append(out_boxes[current_idx])
                aligned_scores.append(out_scores[current_idx])
            else:
                raise ValueError(f"Box not found for alignment: {box}")
        return aligned_prediction, aligned_boxes, aligned_scores

    def predict(self, documents, words: List[List[str]], boxes: List[List[List[int]]], batch_size: Optional[int] = None):
        """transformers.py:302-401.  ``documents``: objects with ``.tensor`` and a ``.tags`` dict — their ``tags["indexer"]`` is
        set and they are returned — or plain frames, for which the per-page dictionaries are returned."""
        if batch_size is None:
            batch_size = self.batch_size
        if len(documents) == 0:
            return documents
        assert words is not None and boxes is not None, "words and boxes must be provided for sequence classification"
        assert len(documents) == len(words) == len(boxes), "documents, words and boxes must have the same length"
        plain = not hasattr(documents[0], "tensor")
        frames = [d if plain else d.tensor for d in documents]
        frames, words, boxes_normal = self.preprocess(frames, words, boxes)
        step = max(int(batch_size), 1)
        tagged = []
        for s in range(0, len(frames), step):
            tagged.extend(self._inference_pages(frames[s:s + step], words[s:s + step], boxes_normal[s:s + step], self.labels))
        annotations = []
        for k, (frame, (true_predictions, true_boxes, true_scores)) in enumerate(zip(frames, tagged)):
            annotations.append({"meta": {"imageSize": {"width": frame.shape[1], "height": frame.shape[0]}, "page": k},
                                "predictions": true_predictions, "boxes": true_boxes, "scores": true_scores})
        results = self.postprocess(frames, annotations, words, boxes, None)
        pages = [{"page": k, "meta": [v for v in results["meta"] if v["page"] == k],
                  "kv": [v for v in results["kv"] if v["page"] == k], "ner": [v for v in results["ner"] if v["page"] == k],
                  "groups": [v for v in results["groups"] if v["page"] == k]} for k in range(len(documents))]
        if plain:
            return pages
        for document, page in zip(documents, pages):
            document.tags["indexer"] = page
        return documents

    def decorate_aggregates_with_text(self, aggregated_kv: List[dict], frames: List[np.ndarray]):
        """transformers.py:403-479: a second read of the found regions (RAW_LINE) for their text, one engine call."""
        regions = []

        def create_region(field_id, page_index, bbox):
            x, y, w, h = np.array(bbox).astype(np.int32)
            return {"id": field_id, "pageIndex": page_index, "x": x, "y": y, "w": w, "h": h}

        for k, agg_result in enumerate(aggregated_kv):
            page_index = int(agg_result["page"])
            category = agg_result["category"]
            if "question" in agg_result["value"]:
                regions.append(create_region(f"{category}_{k}_k", page_index, agg_result["value"]["question"]["bbox"]))
            if "answer" in agg_result["value"]:
                regions.append(create_region(f"{category}_{k}_v", page_index, agg_result["value"]["answer"]["bbox"]))
        if len(regions) == 0:
            return
        from .ocr_engine import CoordinateFormat

        if self.ocr_engine is None:
            raise MarieHipError("TransformersDocumentIndexer needs an ocr_engine to read the text of the regions it finds")
        region_results = self.ocr_engine.extract(frames, PSMode.RAW_LINE, CoordinateFormat.XYWH, regions, **{"filter_snippets": True})
        if "regions" not in region_results:
            return
        region_results = region_results["regions"]
        for k, agg_result in enumerate(aggregated_kv):
            category = agg_result["category"]
            for region in region_results:
                rid = region["id"]
                if rid == f"{category}_{k}_k":
                    agg_result["value"]["question"]["text"] = {"text": region["text"], "confidence": region["confidence"]}
                if rid == f"{category}_{k}_v":
                    agg_result["value"]["answer"]["text"] = {"text": region["text"], "confidence": region["confidence"]}

    def group_composite_entities(self, entities_to_group: List[dict], lines_bboxes, true_predictions: List[str],
                                 true_boxes: List[List[int]], true_scores: List[float], frame) -> Dict[str, Dict[str, EntityGroup]]:
        """transformers.py:703-806."""
        grouped_entities = {}
        for entity in entities_to_group:
            expected_keys = entity["entities"]
            entity_name = entity["name"]
            filtered_predictions, filtered_boxes, filtered_scores = [], [], []
            for prediction, pred_box, pred_score in zip(true_predictions, true_boxes, true_scores):
                if prediction[2:] in expected_keys:
                    filtered_predictions.append(prediction)
                    filtered_boxes.append(pred_box)
                    filtered_scores.append(pred_score)
            groups = self.group_by_line(lines_bboxes, filtered_boxes, filtered_predictions, filtered_scores)
            aggregated_keys = self.aggregate_groups_by_line(expected_keys, groups, lines_bboxes, filtered_boxes,
                                                            filtered_predictions, filtered_scores)
            self.fix_misslabeled_tokens(expected_keys, aggregated_keys)
            last_line, group_id, max_line_diff = 0, 0, 2
            collected_groups: Dict[int, list] = {}
            for key, groups in aggregated_keys.items():
                for group in groups:
                    line_diff = group.line - last_line
                    if last_line != 0 and line_diff > max_line_diff:
                        group_id += 1
                    if group_id not in collected_groups:
                        collected_groups[group_id] = []
                    collected_groups[group_id].append(group)
                    last_line = group.line
            merge_groups: Dict[str, Any] = {}
            for group_id, group in collected_groups.items():
                group = sorted(group, key=lambda x: x.bbox[0])
                bboxes = [g.bbox for g in group]
                visited = [False for _ in range(0, len(bboxes))]
                for idx in range(0, len(bboxes)):
                    if visited[idx]:
                        continue
                    ag_key = f"{group_id}_{idx}"
                    visited[idx] = True
                    overlaps, indexes, scores = find_overlap_horizontal(bboxes[idx], bboxes)
                    merge_groups[ag_key] = [group[idx]]
                    for _, overlap_idx in zip(overlaps, indexes):
                        visited[overlap_idx] = True
                        merge_groups[ag_key].append(group[overlap_idx])
            for key, group in merge_groups.items():
                sorted_group = sorted(group, key=lambda x: x.line)
                component_keys = list(set([g.key for g in sorted_group]))
                block = merge_bboxes_as_block([g.bbox for g in sorted_group])
                merge_groups[key] = EntityGroup(bbox=block, key=f"{entity_name}_{key}", group=sorted_group,
                                                components=component_keys)
            grouped_entities[entity_name] = merge_groups
        return grouped_entities

    def postprocess(self, frames: List[np.ndarray], annotations: List[dict], words: List[List[str]],
                    boxes: List[List[List[int]]], file_hash=None):
        """transformers.py:808-1070.  ``boxes`` are the word boxes in pixels (x, y, w, h)."""
        assert len(annotations) == len(words) == len(boxes) == len(frames)
        aggregated_ner, aggregated_groups, aggregated_kv, aggregated_meta = [], [], [], []
        expected_ner = self.init_configuration["expected_ner"]
        expected_keys = self.init_configuration["expected_keys"]
        expected_pair = self.init_configuration["expected_pair"]
        entities_to_group = self.init_configuration["entities_to_group"]
        entities_to_group_by_name = {entity["name"]: entity for entity in (entities_to_group or [])}
        for i, (_boxes, _words, annotation, frame) in enumerate(zip(boxes, words, annotations, frames)):
            lines_bboxes = line_merge(np.asarray(frame), _boxes)
            true_predictions = annotation["predictions"]
            true_boxes = annotation["boxes"]
            true_scores = annotation["scores"]
            grouped_entities = {}
            if entities_to_group is not None and len(entities_to_group) > 0:
                grouped_entities = self.group_composite_entities(entities_to_group, lines_bboxes, true_predictions, true_boxes,
                                                                 true_scores, frame)
            groups = self.group_by_line(lines_bboxes, true_boxes, true_predictions, true_scores)
            aggregated_keys = self.aggregate_groups_by_line(expected_keys, groups, lines_bboxes, true_boxes, true_predictions,
                                                            true_scores)
            self.fix_misslabeled_tokens(expected_keys, aggregated_keys)
            # field groups that say a field could have been present without being part of a key/value pair
            possible_fields = self.init_configuration["possible_fields"]
            possible_field_meta = {}
            for field in possible_fields.keys():
                fields = possible_fields[field]
                possible_field_meta[field] = {"found": False, "fields": []}
                for k in aggregated_keys.keys():
                    for ner_key in aggregated_keys[k]:
                        key = ner_key.key
                        if key in fields and key not in possible_field_meta[field]["fields"]:
                            possible_field_meta[field]["found"] = True
                            possible_field_meta[field]["fields"].append(key)
            aggregated_meta.append({"page": i, "fields": possible_field_meta})
            # key/value pairs
            for pair in expected_pair:
                expected_question, expected_answer = pair[0], pair[1]
                for k in aggregated_keys.keys():
                    found_key = None
                    found_val = None
                    for ner_key in aggregated_keys[k]:
                        key = ner_key.key
                        if expected_question == key:
                            found_key = ner_key
                            continue
                        if found_key is not None and found_val is None:
                            for exp_key in expected_answer:
                                if key in exp_key:
                                    found_val = ner_key
                                    break
                            if found_val is not None:
                                if found_val.bbox[0] < found_key.bbox[0]:      # the answer is not on the right of the question
                                    continue
                                aggregated_kv.append({"page": i, "category": found_key.key,
                                                      "value": {"question": found_key.__dict__, "answer": found_val.__dict__}})
            # NER tags
            for tag in expected_ner:
                for k in aggregated_keys.keys():
                    for ner_key in aggregated_keys[k]:
                        if ner_key.key == tag:
                            aggregated_ner.append({"page": i, "category": tag, "value": {"answer": ner_key.__dict__}})
            # composite entities
            for entity, groups in grouped_entities.items():
                for group_id, group in groups.items():
                    aggregated_entity_groups = []
                    for item in group.group:
                        aggregated_entity_groups.append({"page": i, "category": f"{entity}_{group_id}_{item.key}",
                                                         "value": {"answer": {"bbox": item.bbox}}})
                    self.decorate_aggregates_with_text(aggregated_entity_groups, frames)
                    entity_texts = "\n".join([item["value"]["answer"]["text"]["text"] for item in aggregated_entity_groups])
                    entity_text_confidence = round(
                        np.average([item["value"]["answer"]["text"]["confidence"] for item in aggregated_entity_groups]), 6)
                    entity_config = entities_to_group_by_name[entity]
                    if "validation" in entity_config and "type" not in entity_config["validation"]:
                        raise ValueError("Validation type not found")
                    # no address validator in this project: what the reference yields when its validator raises
                    aggregated_groups.append({
                        "page": i, "category": entity, "components": group.components,
                        "value": {"answer": {"bbox": group.bbox, "text": {"text": entity_texts, "confidence": entity_text_confidence},
                                             "confidence": 1, "validation": {"validated": False, "text": None}}}})
        self.decorate_aggregates_with_text(aggregated_ner, frames)
        self.decorate_aggregates_with_text(aggregated_kv, frames)
        return {"meta": aggregated_meta, "kv": aggregated_kv, "ner": aggregated_ner, "groups": aggregated_groups}

    def fix_misslabeled_tokens(self, expected_keys: List[str], aggregated_keys: Dict[int, Any]):
        """transformers.py:1072-1124: spans of one key on one line that overlap horizontally are merged into one
        (B-PAN I-PAN I-PAN B-PAN-ANS I-PAN)."""
        if self.init_configuration["mislabeled_token_strategy"] != "aggregate":
            raise NotImplementedError(
                f"Mislabeled token strategy not supported : {self.init_configuration['mislabeled_token_strategy']}")
        for key in expected_keys:
            for ag_key in aggregated_keys.keys():
                row_items = aggregated_keys[ag_key]
                bboxes = [row.bbox for row in row_items if row.key == key]
                visited = [False for _ in range(0, len(bboxes))]
                to_merge = {}
                for idx in range(0, len(bboxes)):
                    if visited[idx]:
                        continue
                    visited[idx] = True
                    overlaps, indexes, scores = find_overlap_horizontal(bboxes[idx], bboxes)
                    to_merge[ag_key] = [idx]
                    for _, overlap_idx in zip(overlaps, indexes):
                        visited[overlap_idx] = True
                        to_merge[ag_key].append(overlap_idx)
                for _k, idxs in to_merge.items():
                    items = np.array(aggregated_keys[_k])
                    if len(idxs) == 1:
                        continue
                    idxs = np.array(idxs)
                    picks = items[idxs]
                    remaining = np.delete(items, idxs)
                    score_avg = round(np.average([item.score for item in picks]), 6)
                    block = merge_bboxes_as_block([item.bbox for item in picks])
                    new_item = picks[0]
                    new_item.score = score_avg
                    new_item.bbox = block
                    aggregated_keys[_k] = np.concatenate(([new_item], remaining))

    def aggregate_groups_by_line(self, expected_keys: List[str], groups: Dict[int, List[int]], lines_bboxes, true_boxes,
                                 true_predictions: List[str], true_scores, visualizer=None) -> dict:
        """transformers.py:1126-1174: per line, the spans of every expected key as ``LineGroup`` (merged box, mean score)."""
        aggregated_keys = {}
        for line_idx, line_box in enumerate(lines_bboxes):
            if line_idx not in groups:
                continue
            line_aggregation = self.group_horizontal_span(expected_keys, groups[line_idx], true_predictions)
            true_boxes = np.array(true_boxes)
            true_scores = np.array(true_scores)
            for line_agg in line_aggregation:
                field = line_agg["key"]
                for group_index in line_agg["groups"]:
                    group_score = round(np.average(true_scores[group_index]), 6)
                    group_bbox = merge_bboxes_as_block(true_boxes[group_index])
                    key_result = LineGroup(line=line_idx, key=field, bbox=group_bbox, score=group_score)
                    if line_idx not in aggregated_keys:
                        aggregated_keys[line_idx] = []
                    aggregated_keys[line_idx].append(key_result)
        return aggregated_keys

    def group_horizontal_span(self, expected_keys: List[str], prediction_indexes: List[int], true_predictions) -> list:
        """transformers.py:1176-1208: runs of consecutive predictions of one key."""
        line_aggregator = []
        for key in expected_keys:
            spans = []
            skip_to = -1
            for m in range(0, len(prediction_indexes)):
                if skip_to != -1 and m <= skip_to:
                    continue
                aggregator = []
                if true_predictions[prediction_indexes[m]][2:] == key:
                    for n in range(m, len(prediction_indexes)):
                        pred_idx = prediction_indexes[n]
                        if true_predictions[pred_idx][2:] != key:
                            break
                        aggregator.append(pred_idx)
                        skip_to = n
                if len(aggregator) > 0:
                    spans.append(aggregator)
            if len(spans) > 0:
                line_aggregator.append({"key": key, "groups": spans})
        return line_aggregator

    def group_by_line(self, lines_bboxes, true_boxes: List[List[int]], true_predictions: List[str], true_scores: List[float]) -> dict:
        """transformers.py:1210-1243: prediction indices by the line number ``find_line_number`` gives their box; 'O' and
        boxes without extent are left out."""
        groups: Dict[int, List[int]] = {}
        for pred_idx, (prediction, pred_box, pred_score) in enumerate(zip(true_predictions, true_boxes, true_scores)):
            if not prediction[2:]:
                continue
            if np.array_equal(pred_box, [0.0, 0.0, 0.0, 0.0]) or (pred_box[2] == 0 and pred_box[3] == 0):
                continue
            line_number = find_line_number(lines_bboxes, pred_box)
            if line_number not in groups:
                groups[line_number] = []
            groups[line_number].append(pred_idx)
        return groups

    def close(self):
        m = getattr(self, "model", None)
        if m is not None and hasattr(m, "close"):
            m.close()
