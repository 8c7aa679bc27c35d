"""CPU checks of the document splitter: the constructor's errors, the ``predict`` / ``run`` surface over the torch restatement
(tag name, pairing of page i with ``words[i]``), and the LANCZOS constant and ``mhip_layoutlmv3_set_resample`` in the header
and the binding."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layoutlmv3_ref as R  # noqa: E402

from marie_icr_amd._lib import MarieHipError  # noqa: E402
from marie_icr_amd.document_classifier import LayoutLMv3PagePredictor, TransformersDocumentClassifier  # noqa: E402
from marie_icr_amd.document_splitter import BaseDocumentSplitter, TransformersDocumentSplitter  # noqa: E402
from marie_icr_amd.weights import make_layoutlmv3_state, write_synthetic_bpe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCED = dict(R.BASE_CFG, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
               coordinate_size=16, shape_size=32, num_labels=3)


class _CpuSplitter(TransformersDocumentSplitter):
    """the surface over the torch restatement instead of the HIP model (no GPU in this file); the image processor's resize
    is Pillow's, with the filter the class names"""

    def _open_model(self, state, ctx):
        self.state, self.calls, self.seen = state, 0, []

    def _logits(self, pages, ids, bbox, mask):
        self.calls += 1
        self.seen.append((ids.copy(), bbox.copy()))
        cfg = dict(R.BASE_CFG, **self.hf_config)
        px = np.stack([np.asarray(Image.fromarray(p).resize((224, 224), self.RESAMPLE)) for p in pages])
        pv = torch.from_numpy((px.astype(np.float64) / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
        return R.forward(self.state, cfg, ids, bbox, mask, pv, torch.float32)[1].numpy()


class _Doc:
    def __init__(self, tensor, id=None):
        self.tensor, self.tags, self.id = tensor, {}, id


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("splitter_cpu")
    vocab = write_synthetic_bpe(str(d), seed=1)
    cfg = dict(REDUCED, vocab_size=len(vocab), id2label={"0": "first", "1": "middle", "2": "last"})
    with open(d / "config.json", "w") as f:
        json.dump(cfg, f)
    state = make_layoutlmv3_state(2, 128, 2, 2, 256, len(vocab), coordinate_size=16, shape_size=32, num_labels=3)
    return str(d), state


def test_constructor_errors(model_dir, tmp_path):
    d, _ = model_dir
    with pytest.raises(MarieHipError, match="GPU only"):
        TransformersDocumentSplitter(d, use_gpu=False)
    with pytest.raises(FileNotFoundError):
        TransformersDocumentSplitter(str(tmp_path / "absent"))
    with pytest.raises(ValueError, match="precision"):
        TransformersDocumentSplitter(d, precision="bf16")
    # the same errors as the classifier
    with pytest.raises(MarieHipError, match="GPU only"):
        TransformersDocumentClassifier(d, use_gpu=False)
    with pytest.raises(ValueError, match="precision"):
        TransformersDocumentClassifier(d, precision="bf16")


def test_the_reference_constructor_arguments_are_accepted(model_dir):
    d, state = model_dir
    sp = _CpuSplitter(d, None, None, True, ["first", "middle", "last"], 4, None, None, True, state=state, precision="f32")
    assert sp.batch_size == 4 and sp.labels == ["first", "middle", "last"] and sp.show_error is True
    assert sp.id2label == {0: "first", 1: "middle", 2: "last"}
    assert isinstance(sp, BaseDocumentSplitter) and isinstance(sp, LayoutLMv3PagePredictor)
    assert not isinstance(sp, TransformersDocumentClassifier) and not hasattr(sp, "task") and not hasattr(sp, "top_k")
    assert sp.TAG == "split" and sp.RESAMPLE == Image.LANCZOS and TransformersDocumentClassifier.RESAMPLE == Image.BILINEAR
    import marie_icr_amd

    assert marie_icr_amd.TransformersDocumentSplitter is TransformersDocumentSplitter


def test_predict_surface_and_pairing(model_dir):
    d, state = model_dir
    sp = _CpuSplitter(d, state=state, precision="f32")
    pages = [R.make_test_pages(8)[i] for i in (5, 7, 6)]   # a large page, the small one, a large page
    frames = [p for p, _, _ in pages]
    words, boxes = [w for _, w, _ in pages], [b for _, _, b in pages]
    with pytest.raises(AssertionError):
        sp.predict(frames)
    with pytest.raises(AssertionError):
        sp.predict(frames, words=words)
    with pytest.raises(AssertionError):
        sp.predict(frames, words[:2], boxes)
    with pytest.raises(AssertionError):
        sp.predict(frames, words, boxes[:1])
    assert sp.run([]) == [] and sp.predict([], [], []) == []
    docs = [_Doc(f, i) for i, f in enumerate(frames)]
    sp.calls, sp.seen = 0, []
    out = sp.run(docs, words, boxes, batch_size=2)
    assert out is docs and sp.calls == 2                   # batches of 2 + 1: one model call each
    # page i went in with words[i] and boxes[i]: the page of the second batch too, which the reference pairs with words[0]
    sent_ids, sent_bbox = (np.concatenate([s[k] for s in sp.seen]) for k in (0, 1))
    for i, (f, w, b) in enumerate(zip(frames, words, boxes)):
        ids, bbox, _ = sp.encode(f, w, b)
        assert np.array_equal(sent_ids[i], ids) and np.array_equal(sent_bbox[i], bbox), i
    assert not np.array_equal(sent_ids[2], sent_ids[0])
    single = [sp.predict_document_image(f, w, b, top_k=3) for f, w, b in zip(frames, words, boxes)]
    for doc, one in zip(docs, single):
        t = doc.tags["split"]
        assert set(doc.tags) == {"split"} and set(t) == {"label", "score", "details"}
        assert t["label"] in ("first", "middle", "last") and 0.0 < t["score"] <= 1.0 and t["details"][t["label"]] == t["score"]
        assert len(one) == 1 and set(one[0]) == {"label", "score"}
        assert one[0]["label"] == t["label"] and abs(one[0]["score"] - t["score"]) <= 1e-5
    plain = sp.predict(frames, words, boxes, batch_size=1)
    assert [p["label"] for p in plain] == [doc.tags["split"]["label"] for doc in docs]


def test_header_and_binding():
    from marie_icr_amd import _lib, layoutlmv3

    text = open(os.path.join(ROOT, "include", "marie_hip.h")).read()
    m = re.search(r"^#define\s+MHIP_PIL_LANCZOS\s+(\d+)", text, flags=re.M)
    assert m and int(m.group(1)) == 1 == int(Image.LANCZOS) == layoutlmv3.PIL_LANCZOS
    assert (layoutlmv3.PIL_BILINEAR, layoutlmv3.PIL_BICUBIC) == (int(Image.BILINEAR), int(Image.BICUBIC))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mhip_layoutlmv3_set_resample\s*\(\s*mhip_layoutlmv3\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    sig = {s[0]: s for s in _lib._SIGNATURES}["mhip_layoutlmv3_set_resample"]
    assert sig[1] is _lib.C.c_int and sig[2] == [_lib.C.c_void_p, _lib.C.c_int]
    assert "mhip_layoutlmv3_set_resample" in _lib.EXPORTED_SYMBOLS
    assert hasattr(layoutlmv3.LayoutLMv3Model, "set_resample")
