"""What tests/make_bert_text_long_golden.py, tests/test_berttext_long_cpu.py and tests/test_berttext_long_gpu.py share: the models
and texts of tests/golden/bert_text_long.npz, its loader, and a float64 attention reference that never builds an npad x npad
matrix."""
import json
import os

import numpy as np

import bert_text_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bert_text_long.npz")
LENS, NPAD = [129, 257, 512], 512
CONFIG_A = dict(R.CONFIG_A, max_position=512)
CONFIG_B = dict(R.CONFIG_B, max_position=512)
CONFIG_B_JINA = dict(R.CONFIG_B_JINA, max_position=512)
CONFIGS = {"A": CONFIG_A, "B": CONFIG_B, "B_jina": CONFIG_B_JINA}


def stored_rows(lens):
    """(n, 4): the rows of every hidden state that the golden keeps"""
    return np.array([[0, 127, 128, n - 1] for n in lens], np.int32)


def load_long_golden(path=GOLDEN):
    """-> {"A" / "B": dict(state, ids, lens, rows (n, 4), hidden_rows (depth + 1, n, 4, dim), mean, mean_norm, cls)}"""
    z = np.load(path)
    models = {}
    for name in ("A", "B"):
        keys = json.loads(str(z[f"{name}/keys"]))
        exps = z[f"{name}/exps"]
        state = {k: (z[f"{name}/w{i}"].astype(np.float64) * 2.0 ** int(exps[i])).astype(np.float32) for i, k in enumerate(keys)}
        models[name] = dict(state=state, **{k: z[f"{name}/{k}"] for k in ("ids", "lens", "rows", "hidden_rows", "mean", "mean_norm", "cls")})
    return models


def take_rows(taps, rows):
    """taps (depth + 1, n, npad, dim), rows (n, 4) -> (depth + 1, n, 4, dim)"""
    return np.asarray(taps)[:, np.arange(len(rows))[:, None], rows]


def attention_blocked(q, k, v, n, slope=None, f16=False, step=512):
    """one sequence, one head: q, k, v float64 (npad, hd), q in log2 units, the first n keys, slope in the same units or None ->
    (npad, hd), `step` queries at a time.  f16 as bert_text_ref.attention: the probabilities (against the row's maximum) rounded
    to float16 as the operand of the second product, their sum not"""
    out = np.zeros_like(q)
    keys = np.arange(n)
    for at in range(0, len(q), step):
        s = q[at:at + step] @ k[:n].T
        if slope is not None:
            s = s - slope * np.abs(np.arange(at, at + len(s))[:, None] - keys[None, :])
        p = np.exp2(s - s.max(-1, keepdims=True))
        out[at:at + step] = ((R.r16(p) if f16 else p) @ v[:n]) / p.sum(-1, keepdims=True)
    return out
