"""CPU checks of the CLIP text side: the tokeniser against transformers.CLIPTokenizer on a synthetic vocabulary, the plain-torch
restatement (tests/cliptext_ref.py, what the GPU tests compare the HIP tower against) against
transformers.CLIPTextModelWithProjection in float64, the checkpoint loader under both key schemes, and the refusals that need
no device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as V  # noqa: E402
import cliptext_ref as R  # noqa: E402

from marie_icr_amd import embeddings as E  # noqa: E402
from marie_icr_amd._lib import MarieHipError  # noqa: E402
from marie_icr_amd.clip_tokenizer import ClipTokenizer  # noqa: E402

# upper case; runs of spaces, tabs and newlines; digits; contractions; punctuation runs; non-ASCII letters in NFD and NFC; the
# empty string; a word with no merge
DESIGNED = ["THE Invoice TOTAL", "the   invoice\t\ttotal\n\n the ", "12 345 total 6", "invoice's total don't", "total!!! ...--(the)",
            "café naïve", "café naïve", "", "xyzzy"]


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    return R.make_vocab(str(tmp_path_factory.mktemp("vocab")))


@pytest.fixture(scope="module")
def tok(vocab):
    return ClipTokenizer.from_files(vocab["vocab"], vocab["merges"])


@pytest.fixture(scope="module")
def hf_tok(vocab):
    from transformers import CLIPTokenizer

    return CLIPTokenizer(vocab["vocab"], vocab["merges"])


# ---------------------------------------------------------------------------------------------------- tokeniser
def test_ids_equal_transformers_on_designed_strings(tok, hf_tok):
    for text in DESIGNED + R.TEXTS:
        got, want = tok.tokenize(text), hf_tok(text)["input_ids"]
        print(repr(text[:40]), got[:12], want[:12])
        assert got == want
    assert tok.tokenize("") == [tok.sot, tok.eot]
    assert len(tok.encode("12 345")) == 5                                   # a digit is a token
    assert tok.tokenize("café") == tok.tokenize("café")          # NFD and NFC agree
    assert tok.encode("the invoice total") == [tok.encoder[w + "</w>"] for w in ("the", "invoice", "total")]


def test_html_entities_are_unescaped_twice(tok):
    amp = tok.encode("&")
    assert len(amp) == 1 and tok.encode("&amp;") == amp and tok.encode("&amp;amp;") == amp


def test_gz_vocabulary_gives_the_same_ids(tok, vocab):
    gz = ClipTokenizer.from_gz(vocab["gz"])
    assert gz.encoder == tok.encoder and gz.bpe_ranks == tok.bpe_ranks
    for text in DESIGNED + R.TEXTS:
        assert gz.tokenize(text) == tok.tokenize(text)
    d = os.path.dirname(vocab["gz"])
    assert ClipTokenizer.from_dir(d).tokenize("the invoice") == tok.tokenize("the invoice")
    assert ClipTokenizer.from_dir(None) is None


def test_context_length_limit(tok):
    ids, eot = tok.encode_batch([" ".join(["invoice"] * 75)])
    assert ids.shape == (1, 80) and eot[0] == 76 and ids[0, 76] == tok.eot and not ids[0, 77:].any()
    with pytest.raises(ValueError, match="78 tokens"):
        tok.tokenize(" ".join(["invoice"] * 76))
    cut = tok.tokenize(" ".join(["invoice"] * 76), truncation=True)
    assert len(cut) == 77 and cut[-1] == tok.eot and cut[0] == tok.sot
    assert set(cut[1:-1]) == {tok.encoder["invoice</w>"]}
    with pytest.raises(ValueError):
        tok.tokenize("the invoice total", context_length=4)


def test_encode_batch_pads_to_a_multiple_of_eight(tok):
    ids, eot = tok.encode_batch(R.TEXTS[:8])
    lengths = [2, 3, 5, 5, 4, 9, 18, 11]
    assert ids.dtype == np.int32 and eot.dtype == np.int32 and ids.shape == (8, 24)
    assert list(eot) == [n - 1 for n in lengths]
    for row, n in zip(ids, lengths):
        assert row[0] == tok.sot and row[n - 1] == tok.eot and not row[n:].any()
    assert tok.encode_batch(["total"])[0].shape == (1, 8) and tok.encode_batch(R.TEXTS)[0].shape == (9, 80)


# ---------------------------------------------------------------------------------------------------- model
def _hf_model(state, cfg, eot_id):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection

    config = CLIPTextConfig(vocab_size=cfg["vocab"], hidden_size=cfg["dim"], intermediate_size=cfg["ffn"],
                            projection_dim=cfg["proj_dim"], num_hidden_layers=cfg["depth"], num_attention_heads=cfg["heads"],
                            max_position_embeddings=cfg["context"], hidden_act="quick_gelu", layer_norm_eps=1e-5,
                            eos_token_id=eot_id, bos_token_id=eot_id - 1, pad_token_id=0)
    model = CLIPTextModelWithProjection(config).double().eval()
    missing, unexpected = model.load_state_dict({k: v.double() for k, v in R.to_transformers(state).items()}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing)
    return model


def test_restatement_equals_transformers_fp64_under_both_key_schemes(tok):
    state = R.make_state(R.SMALL, seed=0)
    ids, eot = tok.encode_batch(R.TEXTS)
    assert [int(e) + 1 for e in eot] == [2, 3, 5, 5, 4, 9, 18, 11, 77]
    ids77 = ids[:, :R.SMALL["context"]]                     # the library has no position past the context
    with torch.no_grad():
        out = _hf_model(state, R.SMALL, tok.eot)(input_ids=torch.from_numpy(ids77).long(), output_hidden_states=True)
    want, want_taps = out.text_embeds.numpy(), torch.stack(out.hidden_states).numpy()
    for name, checkpoint in (("openai", state), ("transformers", R.to_transformers(state)), ("wrapped", {"model_state_dict": state})):
        tensors, cfg = E.load_clip_text_state(checkpoint)
        geometry = {k: getattr(cfg, k) for k in R.SMALL}
        assert geometry == R.SMALL and abs(cfg.ln_eps - 1e-5) < 1e-12
        taps, emb = R.forward(tensors, R.SMALL, ids77, eot, torch.float64)
        err, tap_err = np.abs(emb.numpy() - want).max(), np.abs(taps.numpy() - want_taps).max()
        print(f"{name}: max |d embedding| {err:.3e}, max |d hidden state| {tap_err:.3e} (entries up to {np.abs(want).max():.2f})")
        assert err <= 1e-12 and tap_err <= 1e-12
    # the 80-row layout of the device (zero position rows past the context) gives the same embeddings: the rows are padding
    _, emb80 = R.forward(state, R.SMALL, ids, eot, torch.float64)
    assert np.abs(emb80.numpy() - want).max() <= 1e-12


def test_geometry_is_read_from_shapes_at_vit_b32(tok):
    shapes = R.VIT_B32_TEXT
    D, F = shapes["dim"], shapes["ffn"]
    z = lambda *s: np.zeros(s, np.float16)      # OpenAI checkpoints are fp16
    state = {"token_embedding.weight": z(shapes["vocab"], D), "positional_embedding": z(shapes["context"], D),
             "ln_final.weight": z(D), "ln_final.bias": z(D), "text_projection": z(D, shapes["proj_dim"]), "logit_scale": z()}
    for i in range(shapes["depth"]):
        p = f"transformer.resblocks.{i}."
        state.update({p + "attn.in_proj_weight": z(3 * D, D), p + "attn.in_proj_bias": z(3 * D), p + "attn.out_proj.weight": z(D, D),
                      p + "attn.out_proj.bias": z(D), p + "ln_1.weight": z(D), p + "ln_1.bias": z(D), p + "ln_2.weight": z(D),
                      p + "ln_2.bias": z(D), p + "mlp.c_fc.weight": z(F, D), p + "mlp.c_fc.bias": z(F),
                      p + "mlp.c_proj.weight": z(D, F), p + "mlp.c_proj.bias": z(D)})
    tensors, cfg = E.load_clip_text_state(state)
    assert {k: getattr(cfg, k) for k in shapes} == shapes
    assert "logit_scale" not in tensors and all(v.dtype == np.float32 for v in tensors.values())


def test_vision_only_state_has_no_text_tower():
    vision = V.make_state(V.SMALL, *V.GAINS["small"], seed=0)
    assert E.load_clip_text_state(vision) is None
    assert E.load_clip_text_state(V.to_transformers(vision)) is None
    both = dict(vision, **R.make_state(R.SMALL, seed=0))
    assert E.load_clip_text_state(both) is not None
    tensors, _ = E.load_clip_vision_state(both)             # and the vision loader still takes its own keys only
    assert all(k.startswith("visual.") for k in tensors)


def test_refusals_before_any_device_work(tok):
    vision = V.make_state(V.SMALL, *V.GAINS["small"], seed=0)
    text = R.make_state(R.SMALL, seed=0)
    both = dict(vision, **text)
    with pytest.raises(MarieHipError, match="no text tower"):
        E.ClipImageEmbeddings(state=vision, text=True, tokenizer=tok)
    with pytest.raises(MarieHipError, match="vocabulary"):
        E.ClipImageEmbeddings(state=both, text=True)
    # a text tower that lacks a tensor, and a vocabulary the token table cannot hold
    no_proj = {k: v for k, v in both.items() if k != "text_projection"}
    with pytest.raises(MarieHipError, match="text_projection"):
        E.ClipImageEmbeddings(state=no_proj, tokenizer=tok)
    hf = R.to_transformers(text)
    del hf["text_model.encoder.layers.1.self_attn.k_proj.weight"]
    with pytest.raises(MarieHipError, match="k_proj"):
        E.load_clip_text_state(hf)
    short = dict(both, **{"token_embedding.weight": text["token_embedding.weight"][:100]})
    with pytest.raises(MarieHipError, match="526 entries"):
        E.ClipImageEmbeddings(state=short, tokenizer=tok)
    # an instance without a text side says so
    bare = E.ClipImageEmbeddings.__new__(E.ClipImageEmbeddings)
    with pytest.raises(NotImplementedError, match="text"):
        bare.get_embeddings(["the", "invoice"])
