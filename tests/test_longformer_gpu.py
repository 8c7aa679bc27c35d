"""The Longformer page classifier on the MI355X: attn_window, attn_global_row (marie_icr_amd/csrc/attn_seq.hip) and cls_head
(berttext_ops.hip) alone, the model through mhip_berttext_classify_host and the public classes, against tests/longformer_ref.py —
the float64 set definition that tests/test_longformer_cpu.py pins to transformers' LongformerForSequenceClassification through
tests/golden/longformer.npz.

Bars, those of tests/test_berttext_long_gpu.py:
  * fp32: 1e-3 absolute on O(1) quantities for the kernels, the stream taps and the logits; 1e-4 for scores; 1e-5 for cls_head,
    whose arithmetic is fp32 in both modes;
  * f16: E_ref = max |f16-rounded restatement - float64 restatement| is computed here on the CPU for each case, and
    max |kernel - float64 restatement| <= 2 E_ref;
  * the band is exact and a text's rows do not depend on npad, on its batch or on what lies past its length: bitwise.
Every test prints its figures before it asserts.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_text_ref as R  # noqa: E402
import longformer_ref as L  # noqa: E402
import sentence_families_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16 = 1, 0
HEADS, HD = 2, 64
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    for key in [k for k in _cache if k[0] == "model"]:
        _cache.pop(key).close()
    c.close()


@pytest.fixture(scope="module")
def tc():
    from marie_icr_amd import text_classifier

    return text_classifier


@pytest.fixture(scope="module")
def golden():
    return L.load_golden()


def _qkv(npad, B, seed=0):
    """the input recipe of tests/test_berttext_long_gpu.py: three draws, a ramp over the position on k and over the width on v"""
    rng = np.random.default_rng(7000 + 13 * npad + seed)
    D = HEADS * HD
    q = rng.standard_normal((B, npad, D)) * (R.LOG2E / np.sqrt(HD))
    k = rng.standard_normal((B, npad, D)) + 0.3 * np.linspace(-1, 1, npad)[None, :, None]
    v = rng.standard_normal((B, npad, D)) + np.linspace(-1, 1, D)[None, None, :]
    return [np.ascontiguousarray(a, np.float32) for a in (q, k, v)]


def _read_rows(lens, npad):
    """bool (B, npad): rows 1 .. len - 1, what somebody reads of attn_window's output"""
    r = np.arange(npad)[None, :]
    return (r >= 1) & (r < np.asarray(lens)[:, None])


def _window_batches(w):
    """the lengths of the issue for one-sided window w, cut into batches of at most six texts that share the smallest npad"""
    lens = sorted({2, w + 1, w + 2, 64, 65, 128, 129, 2 * w + 2} | ({1017} if w == 256 else set()))
    out = []
    for at in range(0, len(lens), 6):
        group = lens[at:at + 6]
        out.append(((group[-1] + 7) // 8 * 8, tuple(group)))
    return out


WINDOW_CASES = [(w, npad, lens) for w in (1, 8, 24, 256) for npad, lens in _window_batches(w)]


def _window_ref(w, npad, lens, f16):
    key = ("win", w, npad, f16)
    if key not in _cache:
        q, k, v = _qkv(npad, len(lens))
        if f16:
            out = R.r16(L.window_attention(R.r16(q), R.r16(k), R.r16(v), lens, HEADS, w, f16=True))
        else:
            out = L.window_attention(*(a.astype(np.float64) for a in (q, k, v)), lens, HEADS, w)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- 1. attn_window alone
@pytest.mark.parametrize("w,npad,lens", WINDOW_CASES, ids=[f"w{w}-npad{n}" for w, n, _ in WINDOW_CASES])
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_window_kernel(ctx, tc, precision, w, npad, lens):
    lens = np.array(lens, np.int32)
    q, k, v = _qkv(npad, len(lens))
    want = _window_ref(w, npad, lens, False)
    got = tc.window_attention_host(ctx, precision, q, k, v, lens, HEADS, w)
    rows = _read_rows(lens, npad)
    err = np.abs(got - want)[rows].max()
    if precision == F32:
        print(f"attn_window f32 w {w} npad {npad} lens {lens.tolist()}: max |d| {err:.3e} (outputs up to {np.abs(want[rows]).max():.2f})")
    else:
        e_ref = np.abs(_window_ref(w, npad, lens, True) - want)[rows].max()
        print(f"attn_window f16 w {w} npad {npad} lens {lens.tolist()}: max |d| {err:.3e}, E_ref {e_ref:.3e}")
    assert 0.5 <= np.abs(want[rows]).max() <= 8 and np.isfinite(got).all()
    assert err <= (1e-3 if precision == F32 else 2 * e_ref)


@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_window_band_is_exact(ctx, tc, precision):
    """a key changes the queries within w of it and no other, bit for bit; key 0 changes every query; what lies past a text's
    length, NaN included, changes nothing"""
    w, npad, n = 24, 200, 200
    lens = np.array([n], np.int32)
    q, k, v = _qkv(npad, 1, seed=1)
    base = tc.window_attention_host(ctx, precision, q, k, v, lens, HEADS, w)
    i = np.arange(npad)
    for j in (100, 1, n - 1):
        k2, v2 = k.copy(), v.copy()
        k2[0, j] += 0.5
        v2[0, j] -= 0.75
        got = tc.window_attention_host(ctx, precision, q, k2, v2, lens, HEADS, w)
        inside = (np.abs(i - j) <= w) & (i >= 1)
        same = np.array([np.array_equal(got[0, r], base[0, r]) for r in i])
        print(f"attn_window key {j}: {int((~same[1:]).sum())} rows changed, band holds {int(inside.sum())}")
        assert same[~inside & (i >= 1)].all() and not same[inside].any()
    k2, v2 = k.copy(), v.copy()
    k2[0, 0] += 0.5
    v2[0, 0] -= 0.75
    got = tc.window_attention_host(ctx, precision, q, k2, v2, lens, HEADS, w)
    assert not any(np.array_equal(got[0, r], base[0, r]) for r in range(1, n))
    # rows >= len
    lens = np.array([150], np.int32)
    base = tc.window_attention_host(ctx, precision, q, k, v, lens, HEADS, w)
    k2, v2 = k.copy(), v.copy()
    k2[0, 150:] = np.nan
    v2[0, 150:] = np.nan
    got = tc.window_attention_host(ctx, precision, q, k2, v2, lens, HEADS, w)
    assert np.array_equal(got[0, 1:150], base[0, 1:150]) and np.isfinite(got[0, 1:150]).all()


@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_window_rows_depend_on_the_text_alone(ctx, tc, precision):
    w, n = 24, 150
    q, k, v = _qkv(264, 3, seed=2)
    lens = np.array([97, n, 264], np.int32)
    batch = tc.window_attention_host(ctx, precision, q, k, v, lens, HEADS, w)
    for npad in (152, 200):
        alone = tc.window_attention_host(ctx, precision, *(np.ascontiguousarray(a[1:2, :npad]) for a in (q, k, v)), lens[1:2], HEADS, w)
        assert np.array_equal(alone[0, 1:n], batch[1, 1:n]), f"npad {npad}"


# ---------------------------------------------------------------------------------------------------- 2. attn_global_row alone
@pytest.mark.parametrize("precision", [F32, F16], ids=["f32", "f16"])
def test_attn_global_row_kernel(ctx, tc, precision):
    lens = np.array([1, 2, 127, 128, 129, 1017], np.int32)
    npad = 1024
    q, k, v = _qkv(npad, len(lens), seed=3)
    qg = np.ascontiguousarray(q[:, 0])
    want = L.global_row(*(a.astype(np.float64) for a in (qg, k, v)), lens, HEADS)
    got = tc.global_row_attention_host(ctx, precision, qg, k, v, lens, HEADS)
    err = np.abs(got - want).max()
    if precision == F32:
        print(f"attn_global_row f32: max |d| {err:.3e} (outputs up to {np.abs(want).max():.2f})")
        bar = 1e-3
    else:
        e_ref = np.abs(R.r16(L.global_row(qg.astype(np.float64), R.r16(k), R.r16(v), lens, HEADS)) - want).max()
        print(f"attn_global_row f16: max |d| {err:.3e}, E_ref {e_ref:.3e}")
        bar = 2 * e_ref
    assert 0.5 <= np.abs(want).max() <= 8 and np.isfinite(got).all()
    assert err <= bar
    # what lies past a text's length changes nothing
    k2, v2 = k.copy(), v.copy()
    for b, n in enumerate(lens):
        k2[b, n:] = np.nan
        v2[b, n:] = np.nan
    assert np.array_equal(tc.global_row_attention_host(ctx, precision, qg, k2, v2, lens, HEADS), got)


# ---------------------------------------------------------------------------------------------------- 3. cls_head alone
@pytest.mark.parametrize("function", ["softmax", "sigmoid"])
@pytest.mark.parametrize("labels", [1, 3, 25])
def test_cls_head_kernel(ctx, tc, labels, function):
    rng = np.random.default_rng(50 + labels)
    B, D = 3, 128
    h0 = rng.standard_normal((B, D)).astype(np.float32)
    dw = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    db = (0.2 * rng.standard_normal(D)).astype(np.float32)
    ow = (2.0 * rng.standard_normal((labels, D)) / np.sqrt(D)).astype(np.float32)
    ob = (0.2 * rng.standard_normal(labels)).astype(np.float32)
    want_l, want_s = L.cls_head(h0, dw, db, ow, ob, function)
    got_l, got_s = tc.cls_head_host(ctx, h0, dw, db, ow, ob, tc.HEAD_SOFTMAX if function == "softmax" else tc.HEAD_SIGMOID)
    el, es = np.abs(got_l - want_l).max(), np.abs(got_s - want_s).max()
    print(f"cls_head L {labels} {function}: logits max |d| {el:.3e} (up to {np.abs(want_l).max():.2f}), scores {es:.3e}")
    assert el <= 1e-5 and es <= 1e-5


# ---------------------------------------------------------------------------------------------------- 4. the model
def _model(ctx, tc, name, precision, golden):
    key = ("model", name, precision)
    if key not in _cache:
        m = golden[0][name]
        cfg, windows, labels = tc.longformer_config(L.config_json(m["cfg"]))
        fn = tc.HEAD_SIGMOID if L.head_function(m["cfg"]) == "sigmoid" else tc.HEAD_SOFTMAX
        _cache[key] = tc.TextClassifierModel(ctx, m["state"], cfg, windows, labels, fn, precision)
    return _cache[key]


def _f16_logits(name, golden):
    key = ("f16ref", name)
    if key not in _cache:
        m = golden[0][name]
        _cache[key] = np.stack([L.forward(m["state"], m["cfg"], L.pad_ids([e], (len(e) + 7) // 8 * 8), [len(e)], f16=True)[1][0] for e in m["ids"]])
    return _cache[key]


@pytest.mark.parametrize("name", ["A", "B"])
def test_model_f32_against_the_golden(ctx, tc, golden, name):
    m = golden[0][name]
    model = _model(ctx, tc, name, F32, golden)
    npad = L.MODEL_MAX_LENGTH
    ids = L.pad_ids(m["ids"], npad)
    taps, _ = model.debug_taps_host(ids, m["lens"])
    got_rows = taps[:, np.arange(len(m["lens"]))[:, None], m["rows"]]
    et = np.abs(got_rows - m["tap_rows"]).max(axis=(1, 2, 3))
    logits, scores = model.classify_ids_host(ids, m["lens"])
    el, es = np.abs(logits - m["logits"]).max(), np.abs(scores - m["scores"]).max()
    print(f"longformer {name} f32: taps max |d| {np.array2string(et, precision=2)}, logits {el:.3e}, scores {es:.3e}")
    assert (et <= 1e-3).all() and el <= 1e-3 and es <= 1e-4
    assert np.array_equal(logits.argmax(-1), m["logits"].argmax(-1))
    # embed_host on the windowed handle pools the windowed encoder's rows: the <s> row of the last tap, the same bits
    emb = model.embed_ids_host(ids, m["lens"])
    assert np.array_equal(emb, taps[-1][:, 0])
    # a text's logits do not depend on its batch or on npad, bit for bit
    for i in (0, 6, 10):
        e = m["ids"][i]
        alone, _ = model.classify_ids_host(L.pad_ids([e], (len(e) + 7) // 8 * 8), [len(e)])
        assert np.array_equal(alone[0], logits[i]), f"text {i}"


@pytest.mark.parametrize("name", ["A", "B"])
def test_model_f16_within_twice_the_rounding_of_the_restatement(ctx, tc, golden, name):
    m = golden[0][name]
    model = _model(ctx, tc, name, F16, golden)
    logits, scores = model.classify_ids_host(L.pad_ids(m["ids"], L.MODEL_MAX_LENGTH), m["lens"])
    e_ref = np.abs(_f16_logits(name, golden) - m["logits"]).max()
    err = np.abs(logits - m["logits"]).max()
    ordered = np.sort(m["logits"], -1)
    margin = ordered[:, -1] - ordered[:, -2] if ordered.shape[1] > 1 else np.full(len(ordered), np.inf)
    keep = margin >= 10 * e_ref
    print(f"longformer {name} f16: logits max |d| {err:.3e}, E_ref {e_ref:.3e}; {int(keep.sum())} of {len(keep)} pages kept")
    assert err <= 2 * e_ref
    assert keep.mean() >= 0.75
    assert np.array_equal(logits.argmax(-1)[keep], m["logits"].argmax(-1)[keep])


class _Doc:
    def __init__(self):
        self.tensor, self.tags = None, {}


@pytest.mark.parametrize("name", ["A", "B"])
def test_predict_gives_the_golden_pipelines_labels_and_scores(ctx, golden, tmp_path, name):
    from marie_icr_amd.document_classifier import TransformersDocumentClassifier

    m, texts = golden[0][name], golden[1]
    L.write_model_dir(str(tmp_path), name, m["state"])
    labels = m["cfg"]["num_labels"]
    clf = TransformersDocumentClassifier(str(tmp_path), task="text-classification", top_k=labels, precision="f32", ctx=ctx, batch_size=4)
    docs = [_Doc() for _ in texts]
    words = [t.split(" ") for t in texts]
    assert clf.predict(docs, words, boxes=None) is docs
    worst = 0.0
    for i, d in enumerate(docs):
        c = d.tags["classification"]
        order = np.argsort(-m["scores"][i], kind="stable")
        assert c["label"] == f"LABEL_{order[0]}" and list(c["details"]) == [f"LABEL_{k}" for k in order]
        worst = max(worst, max(abs(c["details"][f"LABEL_{k}"] - m["scores"][i][k]) for k in range(labels)))
        assert c["score"] == c["details"][c["label"]]
    print(f"predict {name}: scores max |d| {worst:.3e}")
    assert worst <= 1e-4
    clf.close()


def test_a_page_of_4096_tokens(ctx, tc, tmp_path):
    """the longest page of longformer-base-4096 at the tiny width: 4096 tokens on a 4098-row position table, window 512"""
    cfg = dict(L.MODELS["A"], max_position=4098, depth=1, attention_window=512)
    S.write_bpe_files(str(tmp_path))
    clf = tc.LongformerTextClassifier(str(tmp_path), state=L.make_state(cfg, 40), config=L.config_json(cfg), precision="f16", ctx=ctx)
    assert clf.max_tokens == clf.model_max_length == 4096
    rng = np.random.default_rng(9)
    ids = [0] + rng.integers(5, cfg["vocab"], 4094).tolist() + [2]
    logits, scores = clf.classify_ids([ids, ids[:9] + [2]])
    print(f"4096 tokens: logits {logits[0].tolist()}, scores {scores[0].tolist()}")
    assert np.isfinite(logits).all() and np.isfinite(scores).all() and abs(scores[0].sum() - 1) <= 1e-5
    # the boundary itself: 4094 words are 4096 tokens and pass as they are, one word more is 4097
    fits, over = " ".join(["the"] * 4094), " ".join(["the"] * 4095)
    assert len(clf.encode(fits, truncation=False)) == 4096 and len(clf.tokenizer.encode(over)) == 4097
    with pytest.raises(ValueError, match="4097 tokens: the position table holds 4096"):
        clf.encode(over, truncation=False)
    cut = clf.encode(over, truncation=True)
    assert len(cut) == 4096 and cut[0] == 0 and cut[-1] == 2 and cut[:-1] == clf.tokenizer.encode(over)[:4095]
    from marie_icr_amd._lib import MarieHipError

    with pytest.raises(MarieHipError, match="rows a text"):      # 4097 ids handed over directly: refused, never clamped
        clf.classify_ids([ids[:-1] + [7, 2]])
    clf.close()


def test_refusals_before_any_launch(ctx, tc, golden):
    from marie_icr_amd._lib import MarieHipError

    m = golden[0]["A"]
    model = _model(ctx, tc, "A", F32, golden)
    ok = L.pad_ids(m["ids"][:2], 16)
    with pytest.raises(MarieHipError, match="rows a text"):
        model.classify_ids_host(L.pad_ids(m["ids"][:2], L.MODEL_MAX_LENGTH + 8), m["lens"][:2])
    with pytest.raises(MarieHipError, match="rows a text"):
        model.classify_ids_host(L.pad_ids(m["ids"][:2], 12), m["lens"][:2])
    for bad in (0, 17):
        with pytest.raises(MarieHipError, match="tokens"):
            model.classify_ids_host(ok, [2, bad])
    for bad in (-1, m["cfg"]["vocab"]):
        ids = ok.copy()
        ids[1, 1] = bad
        with pytest.raises(MarieHipError, match="outside the vocabulary"):
            model.classify_ids_host(ids, m["lens"][:2])
    # a handle without a head
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.embeddings import BertTextModel

    cfg, _, _ = tc.longformer_config(L.config_json(m["cfg"]))
    plain = BertTextModel(ctx, None, cfg, PREC_F32)
    out = np.empty((2, 3), np.float32)
    rc = ctx.lib.mhip_berttext_classify_host(plain.h, ok.ctypes.data, np.array([2, 3], np.int32).ctypes.data, 2, 16, out.ctypes.data, out.ctypes.data)
    assert rc == -1 and b"no classification head" in ctx.lib.mhip_last_error(ctx.h)      # MHIP_ESTATE
    plain.close()


def test_create_refusals_name_their_field(ctx, tc):
    from marie_icr_amd._lib import PREC_F32, MarieHipError

    base = L.config_json(L.MODELS["A"])

    def make(windows=(16, 48), labels=3, fn=1, **changes):
        cfg, _, _ = tc.longformer_config(dict(base, **changes))
        return tc.TextClassifierModel(ctx, None, cfg, windows, labels, fn, PREC_F32)

    for windows, what in (((16, 47), "attention_window 47 of layer 1"), ((0, 48), "attention_window 0 of layer 0"),
                          ((-2, 48), "attention_window -2"), ((16, 1026), "one-sided window of 513")):
        with pytest.raises(MarieHipError, match=what):
            make(windows=windows)
    with pytest.raises(MarieHipError, match="num_labels 0"):
        make(labels=0)
    with pytest.raises(MarieHipError, match="head_function 3"):
        make(fn=3)
    with pytest.raises(MarieHipError, match="head dimension of 32"):
        make(num_attention_heads=4)
    make(windows=(2, 1024)).close()      # the limits themselves are taken
    # finalize names the first missing tensor
    m = make()
    state = {k: v for k, v in L.make_state(L.MODELS["A"], 1).items() if "layer.1.attention.self.key_global.weight" not in k}
    with pytest.raises(MarieHipError, match=r"encoder\.layer\.1\.attention\.self\.key_global\.weight"):
        m.load_state(state)
    m.close()
