"""CPU-side checks of the LayoutReader reading order (marie_icr_amd/layoutreader.py, csrc/layoutreader_api.hip):
  * tests/layoutreader_ref.py, the float64 restatement the GPU tests compare against, reproduces what the model itself computed
    (tests/golden/layoutreader.npz, written by tests/make_layoutreader_golden.py from LayoutlmForSeq2SeqDecoder in float64): the
    decisions are equal and the scores agree to 1e-9.  The restatement caches K / V per layer and skips the pad rows in the
    encoder; the model projects the history again at every step and runs all S rows — so this is also the proof that the two
    formulations agree;
  * the checkpoint loader, the host side of TextLayout.reconstruct (restated by reading text_layout.py: that file imports
    transformers tokenizers and the marie package and cannot be imported here, so its parity is unpinned) and the input refusals;
  * the ABI additions, with the kernel table still at 36 entries;
  * the cap of the f16 margin rule tests/test_layoutreader_gpu.py relies on.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layoutreader_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layoutreader.npz")
NEW_SYMBOLS = ["mhip_layoutreader_create", "mhip_layoutreader_destroy", "mhip_layoutreader_set_tensor", "mhip_layoutreader_finalize",
               "mhip_layoutreader_alloc_arena", "mhip_layoutreader_arena", "mhip_layoutreader_workspace_bytes",
               "mhip_layoutreader_order_host", "mhip_layoutreader_debug_host", "mhip_layoutreader_attention_host"]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def free_run(golden):
    out = R.run_pages(golden["state"], golden["cfg"], golden["pages"])
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def lr():
    from marie_icr_amd import layoutreader

    return layoutreader


# ---------------------------------------------------------------------------------------------------- the restatement
def test_golden_is_the_recipe(golden):
    cfg = golden["cfg"]
    assert cfg == R.CONFIG and [len(p) for p in golden["pages"]] == list(R.PAGE_WORDS)
    T, S = cfg["max_source"] - 2, cfg["max_source"]
    assert golden["decisions"].shape == (4, T) and golden["scores"].shape == (4, T, S)
    sd, _ = R.quantize_state(R.make_state(cfg, R.SEED))
    assert sorted(sd) == sorted(golden["state"]) and all(np.array_equal(sd[k], golden["state"][k]) for k in sd)
    assert all(np.array_equal(a, b) for a, b in zip(R.make_pages(cfg, R.SEED), golden["pages"]))
    m = R.margins(golden["scores"])
    print(f"top-2 margins: min {m.min():.3f}, median {np.median(m):.2f}")
    assert m.min() >= 0.05
    # the decisions reach [SEP] (n + 1) and a pad row: what exercises the >= n handling of reconstruct
    n = np.array(R.PAGE_WORDS)[:, None]
    assert (golden["decisions"] == n + 1).any() and (golden["decisions"] > n + 1).any()


def test_restatement_matches_the_model(golden, free_run):
    """cached K / V and no pad rows in the encoder against re-projection over all S rows"""
    err = float(np.abs(free_run["scores"] - golden["scores"]).max())
    print(f"restatement vs the model: max|dscore| = {err:.2e}, max|demb| = {float(np.abs(free_run['emb'] - golden['emb']).max()):.2e}")
    assert np.array_equal(free_run["decisions"], golden["decisions"])
    assert err <= 1e-9
    assert float(np.abs(free_run["emb"] - golden["emb"]).max()) <= 1e-9


def test_forced_with_own_decisions_equals_free_running(golden, free_run):
    forced = R.run_pages(golden["state"], golden["cfg"], golden["pages"], forced=free_run["decisions"])
    assert np.array_equal(forced["decisions"], free_run["decisions"])
    assert np.array_equal(forced["scores"], free_run["scores"])


def test_forced_feeds_the_forced_row(golden, free_run):
    """forcing another row at step 0 changes step 1 on, and leaves step 0 as it was"""
    page = golden["pages"][1]
    forced = np.array(free_run["decisions"][1])
    forced[0] = 0 if forced[0] != 0 else 1
    out = R.run_page(golden["state"], golden["cfg"], page, forced=forced)
    assert np.array_equal(out["scores"][0], free_run["scores"][1][0])
    assert not np.allclose(out["scores"][1], free_run["scores"][1][1])


def test_f16_margin_rule_keeps_three_quarters_of_the_steps(golden):
    """The f16 GPU test asserts the arg-max only where the golden margin is >= 10 x the score error.  With E_ref from the
    f16-rounded restatement (forced with the golden decisions), the steps below 10 E_ref are at most a quarter of the 128."""
    f16 = R.run_pages(golden["state"], golden["cfg"], golden["pages"], forced=golden["decisions"], f16=True)
    e_ref = float(np.abs(f16["scores"] - golden["scores"]).max())
    m = R.margins(golden["scores"]).ravel()
    share = float((m < 10 * e_ref).mean())
    print(f"E_ref = {e_ref:.4f} on scores within +-{np.abs(golden['scores']).max():.0f}; {share:.1%} of {m.size} steps have a margin below 10 E_ref")
    assert 0 < e_ref < 0.09          # the all-half run of the model is the upper stand-in (0.09)
    assert share <= 0.25


# ---------------------------------------------------------------------------------------------------- loader
def test_loader_key_map_and_dropped_keys(lr, golden):
    cfgj = R.config_json(golden["cfg"])
    ck = dict(golden["state"])
    D = golden["cfg"]["dim"]
    ck["bert.pooler.dense.weight"] = np.zeros((D, D), np.float32)
    ck["cls.seq_relationship.weight"] = np.zeros((2, D), np.float32)
    ck["bert.embeddings.word_embeddings.weight"] = np.zeros((5, D), np.float32)
    # an older checkpoint: gamma / beta
    ck["bert.embeddings.LayerNorm.gamma"] = ck.pop("bert.embeddings.LayerNorm.weight")
    ck["bert.embeddings.LayerNorm.beta"] = ck.pop("bert.embeddings.LayerNorm.bias")
    state, cfg = lr.load_layoutreader_state(ck, cfgj)
    assert (cfg.dim, cfg.heads, cfg.depth, cfg.ffn, cfg.max_source, cfg.max_position, cfg.max_2d) == (128, 2, 2, 256, 34, 68, 1024)
    assert (cfg.source_type, cfg.target_type, cfg.type_vocab) == (0, 1, 2) and abs(cfg.ln_eps - 1e-5) < 1e-12
    assert sorted(state) == sorted(lr.layoutreader_keys(cfg))
    assert not any("pooler" in k or "seq_relationship" in k or "word_embeddings" in k or k.endswith("key.bias") for k in state)
    assert np.array_equal(state["bert.embeddings.LayerNorm.weight"], golden["state"]["bert.embeddings.LayerNorm.weight"])
    assert np.array_equal(state["cls.predictions.bias"], golden["state"]["cls.predictions.bias"])
    # key.bias may be absent altogether: the model never reads it
    lr.load_layoutreader_state({k: v for k, v in golden["state"].items() if not k.endswith("key.bias")}, cfgj)


def test_loader_names_missing_and_misshapen_tensors(lr, golden):
    from marie_icr_amd._lib import MarieHipError

    cfgj = R.config_json(golden["cfg"])
    ck = dict(golden["state"])
    del ck["bert.encoder.layer.1.output.dense.weight"]
    with pytest.raises(MarieHipError, match=r"bert\.encoder\.layer\.1\.output\.dense\.weight"):
        lr.load_layoutreader_state(ck, cfgj)
    ck = dict(golden["state"])
    ck["cls.predictions.bias"] = np.zeros(33, np.float32)
    with pytest.raises(MarieHipError, match=r"cls\.predictions\.bias has shape \(33,\)"):
        lr.load_layoutreader_state(ck, cfgj)
    with pytest.raises(MarieHipError, match="hidden_size"):
        lr.load_layoutreader_state(golden["state"], {k: v for k, v in cfgj.items() if k != "hidden_size"})


@pytest.mark.parametrize("option,value", [("num_qkv", 2), ("seg_emb", True), ("ffn_type", 1), ("relax_projection", 4), ("new_pos_ids", True),
                                          ("base_model_type", "unilm")])
def test_loader_refuses_unbuilt_options(lr, golden, option, value):
    with pytest.raises(NotImplementedError, match=option):
        lr.load_layoutreader_state(golden["state"], dict(R.config_json(golden["cfg"]), **{option: value}))


# ---------------------------------------------------------------------------------------------------- reconstruct
WORDS = ["a", "b", "c", "d"]
BOXES = [[0, 0, 1, 1], [10, 10, 11, 11], [20, 20, 21, 21], [30, 30, 31, 31]]


@pytest.mark.parametrize("idx,order", [
    ([2, 0, 3, 1], [2, 0, 3, 1]),                              # a permutation is taken as it is
    ([2, 2, 0, 0, 3, 1, 1], [2, 0, 3, 1]),                     # duplicates: first seen
    ([1, 1, 1, 1], [1, 0, 2, 3]),                              # missing indices are appended in ascending order
    ([3, 4, 9, 1, 5], [3, 1, 0, 2]),                           # n ([SEP]) and pad rows are dropped
    ([2, -1, 0, 1], [2, 3, 0, 1]),                             # a [CLS] among four distinct indices: fancy indexing takes the last word
    ([0, 1, 2, 3, 4, 4, 4], [0, 1, 2, 3]),
])
def test_reorder_index_lists(lr, idx, order):
    words, boxes = lr.reorder(WORDS, BOXES, idx)
    assert words == [WORDS[i] for i in order] and boxes == [BOXES[i] for i in order]
    assert all(isinstance(b, list) for b in boxes)


def test_reorder_keeps_what_minus_one_does(lr):
    """-1 passes the `idx < len(words)` filter and is not in range(n): with it the list grows past n and the reference's own
    assertion fires.  Reproduced, not repaired."""
    with pytest.raises(AssertionError):
        lr.reorder(WORDS, BOXES, [-1, 0, 1, 2, 3])
    with pytest.raises(AssertionError):
        lr.reorder(WORDS, BOXES, [-1, 0, 0, 0])        # [-1, 0] + unused [1, 2, 3]
    # exactly n distinct indices skip the filter altogether: a [SEP] or pad row among them reaches the fancy indexing
    with pytest.raises(IndexError):
        lr.reorder(WORDS, BOXES, [3, 4, 9, 1, 4])


class _Stub:
    """TextLayout without a model: forward is scripted"""

    def __init__(self, idx, max_len=511):
        self.idx, self.max_len, self.calls = idx, max_len, 0

    def forward(self, words, boxes):
        self.calls += 1
        return self.idx


def test_reconstruct_bypasses_over_long_pages(lr, caplog):
    stub = _Stub([0])
    words, boxes = [str(i) for i in range(512)], [[0, 0, 1, 1]] * 512
    with caplog.at_level("WARNING"):
        out = lr.TextLayout.reconstruct(stub, words, boxes)
    assert out[0] is words and out[1] is boxes and stub.calls == 0
    assert "512 words" in caplog.text and "511" in caplog.text
    stub = _Stub([1, 0, 3, 2])
    assert lr.TextLayout.reconstruct(stub, WORDS, BOXES) == (["b", "a", "d", "c"], [BOXES[1], BOXES[0], BOXES[3], BOXES[2]])
    assert stub.calls == 1


def test_input_refusals(lr):
    ok = lr.check_boxes(BOXES, 32)
    assert ok.dtype == np.int32 and ok.shape == (4, 2 * 2)
    assert lr.check_boxes([], 32).shape == (0, 4)
    for bad in ([[0, 0, 1001, 5]], [[-1, 0, 5, 5]], [[10, 0, 9, 5]], [[0, 10, 5, 9]], [[0, 0, 5]], [[0.5, 0, 5, 5]]):
        with pytest.raises(ValueError):
            lr.check_boxes(bad, 32)
    with pytest.raises(ValueError, match="33 words"):
        lr.check_boxes([[0, 0, 1, 1]] * 33, 32)


def test_no_gpu_fails_loudly(lr, golden):
    from marie_icr_amd._lib import MarieHipError

    with pytest.raises(MarieHipError):
        lr.TextLayout(state=golden["state"], config=R.config_json(golden["cfg"]), use_gpu=False)
    import torch

    if not torch.cuda.is_available():
        import __graft_entry__ as g

        g.build()
        with pytest.raises(MarieHipError):
            lr.TextLayout(state=golden["state"], config=R.config_json(golden["cfg"]))


def test_template_matching_keeps_its_own_text_layout(lr):
    from marie_icr_amd import template_matching

    assert template_matching.TextLayout is not lr.TextLayout


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_additions():
    import __graft_entry__ as g

    g.build()
    from marie_icr_amd import _lib

    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert sorted(s for s in _lib.EXPORTED_SYMBOLS if s.startswith("mhip_layoutreader_")) == sorted(NEW_SYMBOLS)
    # the new kernels are timed under existing slots: the table is not extended
    assert lib.mhip_kernel_count() == 36
    import ctypes as C

    assert C.sizeof(_lib.LayoutReaderConfig) == 11 * 4
