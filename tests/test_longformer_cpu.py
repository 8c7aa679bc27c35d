"""The Longformer page classifier without a GPU: tests/longformer_ref.py (the float64 set definition the GPU tests compare the
kernels with) against what transformers' LongformerForSequenceClassification computed (tests/golden/longformer.npz, written by
tests/make_longformer_golden.py), the tokenisation and truncation of marie_icr_amd/text_classifier.py against LongformerTokenizer's
ids, and the host logic of LongformerTextClassifier / TransformersDocumentClassifier(task="text-classification") over a CPU
stand-in for the model call.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longformer_ref as L  # noqa: E402
import sentence_families_ref as S  # noqa: E402

from marie_icr_amd import text_classifier as TC  # noqa: E402
from marie_icr_amd._lib import MarieHipError  # noqa: E402
from marie_icr_amd.document_classifier import TransformersDocumentClassifier  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return L.load_golden()


@pytest.fixture(scope="module")
def restated(golden):
    """{name: (tap rows, logits)} of the float64 restatement over the golden's texts, each alone, computed once"""
    out = {}
    for name, m in golden[0].items():
        rows, logits = [], []
        for i, e in enumerate(m["ids"]):
            taps, lg = L.forward(m["state"], m["cfg"], L.pad_ids([e], (len(e) + 7) // 8 * 8), [len(e)])
            rows.append(taps[:, 0][:, m["rows"][i]])
            logits.append(lg[0])
        out[name] = (np.stack(rows, 1), np.stack(logits))
    return out


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_set_definition_is_the_librarys_model(golden, restated, name):
    """measured: taps 5.0e-7 / 5.7e-7, logits 9.9e-7 / 6.9e-7 (A / B) — the library's own fp32 soft-max under logit_gain 6"""
    m = golden[0][name]
    rows, logits = restated[name]
    et, el = np.abs(rows - m["tap_rows"]).max(), np.abs(logits - m["logits"]).max()
    print(f"longformer_ref {name}: taps max |d| {et:.2e}, logits {el:.2e}")
    assert m["tap_rows"].shape == (m["cfg"]["depth"] + 1, len(m["lens"]), L.ROWS_PER_TEXT, m["cfg"]["dim"])
    assert et <= 1e-6 and el <= 1e-6
    es = np.abs(L.scores_of(logits, L.head_function(m["cfg"])) - m["scores"]).max()
    assert es <= 1e-6


def test_a_batch_and_its_padding_change_nothing(golden):
    """right-padded in one batch the texts give what each gives alone: pads are nobody's key"""
    m = golden[0]["A"]
    pick = [1, 4, 7, 10]
    ids = L.pad_ids([m["ids"][i] for i in pick], 128)
    taps, logits = L.forward(m["state"], m["cfg"], ids, m["lens"][pick])
    assert np.abs(logits - m["logits"][pick]).max() <= 1e-6


def test_the_golden_covers_the_window_edges(golden):
    lens = golden[0]["A"]["lens"].tolist()
    w = L.windows(L.MODELS["A"])
    assert w == [8, 24] and L.windows(L.MODELS["B"]) == [16, 16]
    assert min(lens) == 2 and max(lens) > 2 * 24 + 2 + 64 and {w[0] + 1, w[0] + 2, w[1] + 1, w[1] + 2, 64, 65} <= set(lens)
    assert len({int(r.argmax()) for r in golden[0]["A"]["logits"]}) > 1      # logit_gain: the labels differ across the texts
    assert os.path.getsize(L.GOLDEN) < 1_000_000


# ---------------------------------------------------------------------------------------------------- CPU stand-ins
class _CpuTextClassifier(TC.LongformerTextClassifier):
    """the class over the float64 restatement instead of the HIP model (no GPU in this file)"""

    def _open_model(self, state, ctx):
        self.state, self.calls, self.model = state, [], None
        self.ref_cfg = dict(dim=self.cfg.dim, heads=self.cfg.heads, depth=self.cfg.depth, ffn=self.cfg.ffn, eps=self.cfg.ln_eps,
                            attention_window=self.hf_config["attention_window"])

    def _rows_budget(self):
        return 4096 * 128

    def _classify_group(self, ids, lens):
        self.calls.append(ids.shape)
        logits = L.forward(self.state, self.ref_cfg, ids, lens)[1]
        fn = {TC.HEAD_SOFTMAX: "softmax", TC.HEAD_SIGMOID: "sigmoid"}[self.head_function]
        return logits.astype(np.float32), L.scores_of(logits, fn).astype(np.float32)


class _CpuDocumentClassifier(TransformersDocumentClassifier):
    def _open_text_model(self, model_dir, tokenizer, state, config, precision, ctx):
        return _CpuTextClassifier(model_dir, tokenizer, state=state, config=config, precision=precision)


class _Doc:
    def __init__(self):
        self.tensor, self.tags = None, {}


def _model_dir(tmp_path, name, **config_changes):
    d = str(tmp_path / name)
    os.makedirs(d, exist_ok=True)
    S.write_bpe_files(d)
    conf = dict(L.config_json(L.MODELS[name]), **config_changes)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(conf, f)
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump(dict(model_max_length=L.MODEL_MAX_LENGTH), f)
    return d, conf


# ---------------------------------------------------------------------------------------------------- tokens
def test_ids_equal_the_tokenizers_truncation_included(golden, tmp_path):
    d, _ = _model_dir(tmp_path, "A")
    clf = _CpuTextClassifier(d, state=golden[0]["A"]["state"])
    assert clf.max_tokens == clf.model_max_length == L.MODEL_MAX_LENGTH
    for text, want in zip(golden[1], golden[0]["A"]["ids"]):
        got = clf.encode(" ".join(text.split(" ")), truncation=True)
        assert got == want.tolist()
    long_text = golden[1][-1]
    assert len(clf.tokenizer.encode(long_text)) == L.TEXT_TOKENS[-1] > L.MODEL_MAX_LENGTH
    with pytest.raises(ValueError, match="230 tokens"):
        clf.encode(long_text, truncation=False)
    # without tokenizer_config.json the position table is the limit
    os.remove(os.path.join(d, "tokenizer_config.json"))
    assert _CpuTextClassifier(d, state=golden[0]["A"]["state"]).model_max_length == L.MODELS["A"]["max_position"] - 2


# ---------------------------------------------------------------------------------------------------- host logic
def test_predict_top_k_order_details_and_labels(golden, tmp_path):
    m, texts = golden[0]["A"], golden[1]
    d, _ = _model_dir(tmp_path, "A")
    words = [t.split(" ") for t in texts]
    clf = _CpuDocumentClassifier(d, task="text-classification", top_k=2, state=m["state"])
    docs = [_Doc() for _ in texts]
    assert clf.predict(docs, words, boxes=[[] for _ in texts]) is docs
    for i, doc in enumerate(docs):
        c = doc.tags["classification"]
        order = np.argsort(-m["scores"][i], kind="stable")[:2]
        assert set(c) == {"label", "score", "details"} and c["label"] == f"LABEL_{order[0]}"
        assert list(c["details"]) == [f"LABEL_{k}" for k in order]                  # sorted by score, cut to top_k
        assert all(abs(c["details"][f"LABEL_{k}"] - m["scores"][i][k]) <= 1e-6 for k in order) and c["score"] == c["details"][c["label"]]
    # plain inputs: the predictions come back; page i has its own list at any batch size
    one = clf.predict(texts, words, batch_size=1)
    four = clf.predict(texts, words, batch_size=4)
    assert one == four == [doc.tags["classification"] for doc in docs]
    assert clf.predict([], [], []) == []
    # id2label with string keys renames LABEL_n as the reference does
    named = _CpuDocumentClassifier(d, task="text-classification", top_k=1, state=m["state"], id2label={"0": "invoice", "1": "letter", "2": "form"})
    assert named.id2label == {0: "invoice", 1: "letter", 2: "form"}
    got = named.predict(texts, words)
    assert [g["label"] for g in got] == [("invoice", "letter", "form")[int(r.argmax())] for r in m["scores"]]
    assert all(list(g["details"]) == [g["label"]] for g in got)
    # the model's own labels of another form are mapped by their index
    d2, _ = _model_dir(tmp_path, "A", id2label={"0": "x", "1": "y", "2": "z"})
    own = _CpuDocumentClassifier(d2, task="text-classification", state=m["state"])
    assert [g["label"] for g in own.predict(texts, words)] == ["xyz"[int(r.argmax())] for r in m["scores"]]
    renamed = _CpuDocumentClassifier(d2, task="text-classification", state=m["state"], id2label={0: "a", 1: "b", 2: "c"})
    assert [g["label"] for g in renamed.predict(texts, words)] == ["abc"[int(r.argmax())] for r in m["scores"]]


def test_calls_are_length_buckets_and_do_not_change_a_page(golden, tmp_path):
    m = golden[0]["A"]
    d, _ = _model_dir(tmp_path, "A")
    clf = _CpuTextClassifier(d, state=m["state"])
    logits, scores = clf.classify_ids([e.tolist() for e in m["ids"]], chunk=4)
    assert clf.calls == [(4, 16), (4, 56), (4, 168), (1, 192)]      # sorted by length, four a call, npad the longest rounded up to 8
    assert np.abs(logits - m["logits"]).max() <= 1e-5 and np.abs(scores - m["scores"]).max() <= 1e-6
    empty = clf.classify_ids([])
    assert empty[0].shape == (0, 3)


def test_sigmoid_softmax_and_regression(golden, tmp_path):
    m, texts = golden[0]["B"], golden[1]
    d, conf = _model_dir(tmp_path, "B")
    clf = _CpuTextClassifier(d, state=m["state"])
    assert clf.head_function == TC.HEAD_SIGMOID and clf.num_labels == 1
    out = clf(texts[:5], top_k=1)
    assert all(len(o) == 1 and o[0]["label"] == "LABEL_0" and abs(o[0]["score"] - m["scores"][i][0]) <= 1e-6 for i, o in enumerate(out))
    assert TC.head_function_of(dict(conf, problem_type="multi_label_classification"), 3) == TC.HEAD_SIGMOID
    assert TC.head_function_of(dict(conf, problem_type="single_label_classification"), 3) == TC.HEAD_SOFTMAX
    assert TC.head_function_of(conf, 3) == TC.HEAD_SOFTMAX
    with pytest.raises(ValueError, match="regression"):
        _CpuTextClassifier(d, state=m["state"], config=dict(conf, problem_type="regression"))
    assert TC.top_k_entries([0.2, 0.5, 0.5], {0: "a", 1: "b", 2: "c"}, None) == [
        {"label": "b", "score": 0.5}, {"label": "c", "score": 0.5}, {"label": "a", "score": 0.2}]


def test_tasks_and_model_types(golden, tmp_path):
    d, conf = _model_dir(tmp_path, "A")
    with pytest.raises(NotImplementedError, match="'bert'"):
        TransformersDocumentClassifier(d, task="text-classification", config=dict(conf, model_type="bert"))
    bert, _ = _model_dir(tmp_path, "B", model_type="bert")
    with pytest.raises(NotImplementedError, match="'bert'"):
        TransformersDocumentClassifier(bert, task="text-classification")
    with pytest.raises(NotImplementedError, match="zero-shot"):
        TransformersDocumentClassifier(d, task="zero-shot-classification")
    with pytest.raises(MarieHipError):
        TransformersDocumentClassifier(d, task="text-classification", use_gpu=False)
    with pytest.raises(ValueError, match="unknown task"):
        TransformersDocumentClassifier(d, task="summarization")
    with pytest.raises(ValueError, match="attention_window"):
        TC.longformer_config(dict(conf, attention_window=[16]))


# ---------------------------------------------------------------------------------------------------- the f16 GPU test's rule
def test_f16_margin_rule_keeps_three_quarters_of_the_test_pages(golden):
    """The f16 GPU test may set aside pages whose float64 top-2 margin is below 10 x the f16 logit error, at most 25 % of them.
    With the seeded weights' logit_gain the restatement alone keeps >= 75 %: the stand-in for the f16 error is the logit
    difference between the float64 restatement and the same restatement with every f16 value of the build rounded."""
    m = golden[0]["A"]
    f16 = np.stack([L.forward(m["state"], m["cfg"], L.pad_ids([e], (len(e) + 7) // 8 * 8), [len(e)], f16=True)[1][0] for e in m["ids"]])
    e16 = np.abs(f16 - m["logits"]).max()
    ordered = np.sort(m["logits"], -1)
    margin = ordered[:, -1] - ordered[:, -2]
    keep = margin >= 10 * e16
    print(f"f16 stand-in error {e16:.2e}; margins {np.round(margin, 2).tolist()}; kept {int(keep.sum())} of {len(keep)}")
    assert keep.mean() >= 0.75
    assert np.array_equal(f16.argmax(-1)[keep], m["logits"].argmax(-1)[keep])


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_symbols_and_config_layout():
    from marie_icr_amd import _lib

    lib = _lib.load()
    for name in ("create_cls", "classify_host", "attention_window_host", "attention_global_host", "cls_head_host"):
        assert f"mhip_berttext_{name}" in _lib.EXPORTED_SYMBOLS and hasattr(lib, f"mhip_berttext_{name}")
    names = [lib.mhip_kernel_name(k).decode() for k in range(lib.mhip_kernel_count())]
    # no profiler slots of their own: the new kernels are counted in attn_short and berttext_pool
    assert {"attn_short", "berttext_pool"} <= set(names) and not any("window" in n or "global" in n or "cls" in n for n in names)
    T = _lib.TextClassifierConfig
    assert [f for f, _ in T._fields_] == ["ex", "attention_window", "num_labels", "head_function"]
    assert T.ex.offset == 0 and T.attention_window.offset == 64 and ctypes.sizeof(T) == 80      # 15 ints, padding, a pointer, 2 ints
