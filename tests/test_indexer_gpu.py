"""GPU parity of the document indexer's model call through the C ABI: the token-head kernel alone against an fp64 evaluation,
windows that share a page against one-window calls bitwise, the fp32 model against the fp32 torch restatement at full size,
the f16 mode under the margin rule, and the two head kinds against the classifier entry points."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indexer_ref as IR  # noqa: E402
import layoutlmv3_ref as R  # noqa: E402

from marie_icr_amd.document_classifier import ByteLevelBPE  # noqa: E402
from marie_icr_amd.weights import make_indexer_config, make_layoutlmv3_token_state, write_synthetic_bpe  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_BAR = 1e-3                 # the project's standing fp32 bar
# 2 x the maximum measured once on an MI355X against the fp32 restatement (the factor 2 covers the run-to-run and seed-to-seed
# spread of a rounding-error maximum); the measurement is recorded in DESIGN.md §0.
F16_TOKEN_LOGIT_ERR_MEASURED = 7.05e-2  # f16 token logits vs the fp32 restatement, max over the valid tokens of the six test windows
MARGIN_FACTOR = 10              # the project's margin rule
SET_ASIDE_CAP = 0.25
HEAD_GAIN = 24.0


@pytest.fixture(scope="module")
def ctx():
    from marie_icr_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ the head kernel alone
def _head_case(rows, D, L, dense, seed):
    rng = np.random.default_rng(seed)
    hidden = rng.standard_normal((rows, D)).astype(np.float32)
    out_w = (rng.uniform(-1, 1, (L, D)) * 8.0 * np.sqrt(3.0 / D)).astype(np.float32)
    out_b = rng.uniform(-0.1, 0.1, L).astype(np.float32)
    dense_w = dense_b = None
    if dense:
        dense_w = (rng.uniform(-1, 1, (D, D)) * np.sqrt(3.0 / D)).astype(np.float32)
        dense_b = rng.uniform(-0.1, 0.1, D).astype(np.float32)
    return hidden, out_w, out_b, dense_w, dense_b


def _head_fp64(hidden, out_w, out_b, dense_w, dense_b):
    x = hidden.astype(np.float64)
    if dense_w is not None:
        x = np.tanh(x @ dense_w.astype(np.float64).T + dense_b)
    z = x @ out_w.astype(np.float64).T + out_b
    e = np.exp(z - z.max(1, keepdims=True))
    return z, z.argmax(1), 1.0 / e.sum(1)


def _max_labels(D):
    return int(min(64, (163840 - 16 * D) // (4 * (D + 8))))


HEAD_SHAPES = [(256, 2), (256, 9), (768, 10), (768, 13), (768, _max_labels(768))]


@pytest.mark.parametrize("D,L", HEAD_SHAPES)
@pytest.mark.parametrize("rows", [1, 63, 65, 512 + 8])
def test_token_head_kernel_fp32_vs_fp64(ctx, rows, D, L):
    """Both head kinds at every shape.  Labels are exact where the fp64 margin exceeds the fp32 bar; scores and logits are
    within the bar."""
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.layoutlmv3 import token_head_host

    for dense in (False, True):
        case = _head_case(rows, D, L, dense, 1000 * rows + L)
        labels, scores, logits = token_head_host(ctx, PREC_F32, case[0], case[1], case[2], case[3], case[4])
        z, lab, sc = _head_fp64(*case)
        top = np.sort(z, axis=1)
        clear = (top[:, -1] - top[:, -2]) > FP32_BAR
        d_z, d_s = float(np.abs(logits - z).max()), float(np.abs(scores - sc).max())
        print(f"token head rows={rows} D={D} L={L} {'dense' if dense else 'linear'}: max|d logits| = {d_z:.3e}, "
              f"max|d score| = {d_s:.3e}, {int(clear.sum())} of {rows} rows clear the bar")
        assert np.isfinite(logits).all() and d_z <= FP32_BAR and d_s <= FP32_BAR
        assert np.array_equal(labels[clear], lab[clear])
        assert ((labels >= 0) & (labels < L)).all()
        # without the logits the decision is the same
        l2, s2, none = token_head_host(ctx, PREC_F32, case[0], case[1], case[2], case[3], case[4], want_logits=False)
        assert none is None and np.array_equal(l2, labels) and np.array_equal(s2, scores)


def test_token_head_ties_take_the_lowest_index(ctx):
    """Exact ties: label rows of W_o repeated, so equal logits are computed by the same instructions on the same numbers."""
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.layoutlmv3 import token_head_host

    D, L, rows = 256, 13, 70
    hidden, out_w, out_b, _, _ = _head_case(rows, D, L, False, 7)
    out_w[9] = out_w[2]; out_w[11] = out_w[2]; out_w[12] = out_w[5]
    out_b[9] = out_b[11] = out_b[2]; out_b[12] = out_b[5]
    labels, scores, logits = token_head_host(ctx, PREC_F32, hidden, out_w, out_b)
    assert np.array_equal(logits[:, 9], logits[:, 2]) and np.array_equal(logits[:, 11], logits[:, 2])
    assert np.array_equal(labels, logits.argmax(1))           # numpy, as torch.argmax, returns the lowest index of the maximum
    tied = np.isin(logits.argmax(1), (2, 5))
    assert tied.sum() >= 5 and not np.isin(labels, (9, 11, 12)).any()
    z, _, sc = _head_fp64(hidden, out_w, out_b, None, None)
    assert float(np.abs(scores - sc).max()) <= FP32_BAR


def test_more_labels_than_the_head_covers_are_refused_for_tagging_only(ctx, case):
    """One label more than the token head covers: the indexer refuses at construction, a linear-head model at finalize, a
    dense-head model at the tag call, each with a message; the same dense-head model still classifies pages (the row-0 head
    has no such limit), with logits equal to the head evaluated in fp64 on the model's own hidden states."""
    from marie_icr_amd._lib import MarieHipError, PREC_F32
    from marie_icr_amd.document_indexer import TransformersDocumentIndexer

    most = ctx.lib.mhip_layoutlmv3_max_token_labels(768)
    assert most == _max_labels(768) and ctx.lib.mhip_layoutlmv3_max_token_labels(1024) == _max_labels(1024)
    L = most + 1
    marie = dict(case["marie"], labels=[f"L{i}" for i in range(L)])
    with pytest.raises(MarieHipError, match="num_labels"):
        TransformersDocumentIndexer(case["dir"], state=case["state"], config=case["cfg"], init_configuration=marie, precision="f32", ctx=ctx)
    with pytest.raises(MarieHipError, match="num_labels"):
        _model(ctx, make_layoutlmv3_token_state(3, L, head="linear", layers=2), PREC_F32, layers=2, num_labels=L)
    state = make_layoutlmv3_token_state(3, L, layers=2)
    m = _model(ctx, state, PREC_F32, layers=2, num_labels=L)
    pages = [p for p, _, _ in case["pages"]]
    with pytest.raises(MarieHipError, match="num_labels"):
        m.tag_host(pages, case["wp"], case["ids"], case["bbox"], case["mask"])
    sel = [0, 1, 3]
    out = m.forward_host(pages, case["ids"][sel], case["bbox"][sel], case["mask"][sel], want_hidden=True)
    m.close()
    x = out["hidden"][:, 0].astype(np.float64)
    z = np.tanh(x @ state["classifier.dense.weight"].astype(np.float64).T + state["classifier.dense.bias"])
    z = z @ state["classifier.out_proj.weight"].astype(np.float64).T + state["classifier.out_proj.bias"]
    d = float(np.abs(out["logits"] - z).max())
    print(f"classify with {L} labels: max|d logits| = {d:.3e}")
    assert out["logits"].shape == (3, L) and d <= FP32_BAR


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """three seeded pages with 1 + 2 + 3 windows (the second window of page 1 mostly padding), their encoding, a 13-label
    dense-head state and the fp32 restatement's token logits"""
    d = tmp_path_factory.mktemp("bpe")
    write_synthetic_bpe(str(d), seed=1)
    tok = ByteLevelBPE(str(d / "vocab.json"), str(d / "merges.txt"))
    pages = IR.make_index_pages(tok)
    wp, ids, bbox, mask, first, norm = IR.encode_index_pages(pages, tok)
    assert wp.tolist() == [0, 1, 1, 2, 2, 2] and mask[2].sum() < 256 and mask[1].sum() == 512
    marie = make_indexer_config(0, 2)
    L = len(marie["labels"])
    state = make_layoutlmv3_token_state(0, L, head_gain=HEAD_GAIN)
    assert IR.head_kind(state) == "dense"
    cfg = dict(R.BASE_CFG, num_labels=L)
    pv, _ = R.pixel_values_from_pages([p for p, _, _ in pages])
    with torch.no_grad():
        logits = IR.forward(state, cfg, ids, bbox, mask, pv[torch.as_tensor(wp).long()], torch.float32)[1].numpy()
    return dict(dir=str(d), tok=tok, pages=pages, wp=wp, ids=ids, bbox=bbox, mask=mask, first=first, norm=norm, marie=marie,
                state=state, cfg=cfg, logits=logits)


def _model(ctx, state, prec, **over):
    from marie_icr_amd.layoutlmv3 import LayoutLMv3Model, default_config

    return LayoutLMv3Model(ctx, state, default_config(ctx.lib, **over), prec)


@pytest.mark.parametrize("num_labels", [7, 13])
def test_windows_that_share_a_page_equal_one_window_calls_bitwise_fp32(ctx, case, num_labels):
    """1 + 2 + 3 windows over three pages in one call against the six windows as six calls, each with its own copy of the
    page: base widths, 2 layers, the linear (7) and the dense (13) head."""
    from marie_icr_amd._lib import PREC_F32

    state = make_layoutlmv3_token_state(3, num_labels, layers=2)
    assert IR.head_kind(state) == ("linear" if num_labels < 10 else "dense")
    m = _model(ctx, state, PREC_F32, layers=2, num_labels=num_labels)
    imgs = [p for p, _, _ in case["pages"]]
    shared = m.tag_host(imgs, case["wp"], case["ids"], case["bbox"], case["mask"], want_logits=True)
    quiet = m.tag_host(imgs, case["wp"], case["ids"], case["bbox"], case["mask"])
    assert np.array_equal(quiet["labels"], shared["labels"]) and np.array_equal(quiet["scores"], shared["scores"])
    for w, p in enumerate(case["wp"].tolist()):
        one = m.tag_host([imgs[p]], [0], case["ids"][w:w + 1], case["bbox"][w:w + 1], case["mask"][w:w + 1], want_logits=True)
        for k in ("labels", "scores", "logits"):
            assert np.array_equal(one[k][0], shared[k][w]), (w, k)
    m.close()
    assert np.isfinite(shared["logits"]).all()
    assert np.array_equal(shared["labels"], shared["logits"].argmax(-1))


def test_fp32_model_equals_the_restatement_at_full_size(ctx, case):
    from marie_icr_amd._lib import PREC_F32
    from marie_icr_amd.document_indexer import TransformersDocumentIndexer

    valid = case["mask"].astype(bool)
    m = _model(ctx, case["state"], PREC_F32, num_labels=case["cfg"]["num_labels"])
    out = m.tag_host([p for p, _, _ in case["pages"]], case["wp"], case["ids"], case["bbox"], case["mask"], want_logits=True)
    m.close()
    d_l = float(np.abs(out["logits"] - case["logits"])[valid].max())
    ref_pred, ref_prob = IR.decide(case["logits"])
    top = np.sort(case["logits"], axis=-1)
    clear = valid & ((top[..., -1] - top[..., -2]) > FP32_BAR)
    d_s = float(np.abs(out["scores"] - ref_prob)[valid].max())
    print(f"fp32 tagger: max|d logits| (valid tokens) = {d_l:.3e}, max|d score| = {d_s:.3e}, "
          f"{int(clear.sum())} of {int(valid.sum())} tokens clear the bar")
    assert d_l <= FP32_BAR and d_s <= FP32_BAR
    assert np.array_equal(out["labels"][clear], ref_pred[clear])
    # the class surface: inference per word against the restatement's, on every word whose decisions clear the bar
    idx = TransformersDocumentIndexer(case["dir"], state=case["state"], config=case["cfg"], init_configuration=case["marie"],
                                      precision="f32", ctx=ctx)
    at = 0
    for k_page, ((page, words, boxes), norm) in enumerate(zip(case["pages"], case["norm"])):
        n = int((case["wp"] == k_page).sum())
        h, w = page.shape[:2]
        sl = slice(at, at + n)
        want = IR.post_model(case["marie"]["labels"], words, norm, w, h, case["logits"][sl], case["bbox"][sl], case["first"][sl])
        got = idx.inference(page, words, norm, case["marie"]["labels"], 0.5)
        assert got[1] == want[1] and len(got[0]) == len(words)
        # a word is compared when every token that carries its box clears the bar (the merge picks among them by score)
        unclear = {tuple(int(c) for c in case["bbox"][sl][i, j]) for i, j in zip(*np.nonzero(~clear[sl] & valid[sl]))}
        same = checked = 0
        for k, nb in enumerate(norm):
            if tuple(nb) in unclear:
                continue
            checked += 1
            same += got[0][k] == want[0][k] and abs(got[2][k] - want[2][k]) <= FP32_BAR
        print(f"page with {n} window(s): {checked} of {len(words)} words compared")
        assert checked >= 0.9 * len(words) and same == checked
        at += n
    idx.close()


def test_f16_mode_keeps_the_labels_under_the_margin_rule(ctx, case):
    from marie_icr_amd._lib import PREC_F16

    valid = case["mask"].astype(bool)
    m = _model(ctx, case["state"], PREC_F16, num_labels=case["cfg"]["num_labels"])
    out = m.tag_host([p for p, _, _ in case["pages"]], case["wp"], case["ids"], case["bbox"], case["mask"], want_logits=True)
    m.close()
    ref = case["logits"]
    err = np.abs(out["logits"] - ref).max(-1)
    print("f16 tagger: max|d logits| per window (valid tokens) =", [float(err[w][valid[w]].max()) for w in range(len(err))])
    assert F16_TOKEN_LOGIT_ERR_MEASURED is not None, "the f16 token-logit error has not been measured on an MI355X yet"
    bound = 2 * F16_TOKEN_LOGIT_ERR_MEASURED
    print(f"bound {bound:.3e}")
    assert np.isfinite(out["logits"]).all() and float(err[valid].max()) <= bound
    top = np.sort(ref, axis=-1)
    kept = valid & ((top[..., -1] - top[..., -2]) > MARGIN_FACTOR * F16_TOKEN_LOGIT_ERR_MEASURED)
    aside = 1.0 - kept.sum() / valid.sum()
    print(f"tokens set aside by the margin rule: {aside:.3f}")
    assert aside <= SET_ASIDE_CAP
    assert np.array_equal(out["labels"][kept], ref.argmax(-1)[kept])
    assert np.array_equal(out["labels"], out["logits"].argmax(-1))


def test_head_kinds_and_the_classifier_entry_points(ctx, case):
    """A dense-head model serves both tasks, and tagging leaves no state behind: its classify answer afterwards is bit for bit
    that of a model, built from the same code, that never tagged.  (Equality of the classifier with its earlier self is not
    shown here: it rests on the classifier's own tests against the restatement.)  A linear-head model refuses classify."""
    from marie_icr_amd._lib import MarieHipError, PREC_F32

    pages = [p for p, _, _ in case["pages"]]
    sel = [0, 1, 3]                                   # the first window of every page: one window a page for classify
    ids, bbox, mask = case["ids"][sel], case["bbox"][sel], case["mask"][sel]
    state = make_layoutlmv3_token_state(3, 13, layers=2)
    fresh = _model(ctx, state, PREC_F32, layers=2, num_labels=13)
    want = fresh.forward_host(pages, ids, bbox, mask, want_hidden=True)
    fresh.close()
    m = _model(ctx, state, PREC_F32, layers=2, num_labels=13)
    tagged = m.tag_host(pages, case["wp"], case["ids"], case["bbox"], case["mask"], want_logits=True)
    got = m.forward_host(pages, ids, bbox, mask, want_hidden=True)
    m.close()
    assert np.array_equal(got["logits"], want["logits"]) and np.array_equal(got["hidden"], want["hidden"])
    # the tagger's logits are the head on the same hidden states
    T = ids.shape[1]
    z = IR.token_logits(state, torch.from_numpy(want["hidden"][:, :T]).double()).numpy()
    d = float(np.abs(tagged["logits"][sel] - z).max())
    print(f"token head on the model's own hidden states: max|d logits| = {d:.3e}")
    assert d <= FP32_BAR
    lin = _model(ctx, make_layoutlmv3_token_state(3, 7, layers=2), PREC_F32, layers=2, num_labels=7)
    with pytest.raises(MarieHipError, match="linear token head"):
        lin.forward_host(pages, ids, bbox, mask)
    packed = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    from marie_icr_amd.layoutlmv3 import pack_pages

    with pytest.raises(MarieHipError, match="linear token head"):
        lin.classify_device(packed.data_ptr(), pack_pages([pages[0][:64, :64].copy()])[1], 1, ids[:1], bbox[:1], mask[:1])
    assert lin.tag_host(pages, case["wp"], case["ids"], case["bbox"], case["mask"])["labels"].max() < 7
    lin.close()
