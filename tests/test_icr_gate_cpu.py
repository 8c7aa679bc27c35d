"""No GPU: the per-step gate of tests/test_icr_gpu.py sets aside at most a quarter of the steps on every input that file uses —
computed from the reference alone (the goldens' logits, the oracle's), so the GPU comparisons there always compare."""
import os

import numpy as np
import pytest

import test_icr_gpu as T
from marie_icr_amd.weights import make_crnn_input, make_icr_state

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _share(ref, tol):
    return 1.0 - T.first_unsafe_step(ref, tol).sum() / (ref.shape[0] * ref.shape[1])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_goldens_keep_within_the_quarter(tag):
    g = np.load(os.path.join(GOLD, f"icr_attn_{tag}.npz"))
    share = _share(g["logits"], 2e-3)
    print(f"golden {tag}: {share:.3f} of the steps set aside")
    assert share <= T.QUARTER
    k = T.first_unsafe_step(g["logits"], 2e-3)
    assert (k >= T.steps_the_text_needs(g["argmax"], T.CRNN_CHARSET)).any()


def test_first_unsafe_step():
    ref = np.zeros((3, 4, 5), np.float32)
    ref[:, :, 0] = 1.0                       # margin 1 everywhere
    ref[1, 2, 1] = 0.999                     # crop 1: margin 1e-3 at step 2
    ref[2, 0, 3] = 1.0                       # crop 2: a tie at step 0
    assert T.first_unsafe_step(ref, 2e-3).tolist() == [4, 2, 0]
    assert T.steps_the_text_needs(np.array([[5, 1, 7], [5, 6, 7], [0, 1, 1]]), T.CRNN_CHARSET).tolist() == [2, 3, 3]


def test_oracle_keeps_within_the_quarter():
    from oracle import crnn_numpy
    from oracle import pil_resample as pr
    from oracle.icr_torch import TorchIcrOracle

    ref = TorchIcrOracle(make_icr_state(2)).logits(crnn_numpy.normalize_u8(make_crnn_input(T.F16_CROP_SEED, 37, 32, 100)))
    assert T.F16_ERR0_BUDGET <= 0.02 * max(1.0, np.abs(ref).max())          # inside what test_f16_vs_oracle allows the first step
    for err0 in (0.0, 0.01, 0.02, T.F16_ERR0_BUDGET):
        share = _share(ref, err0 * 4 + 1e-3)
        print(f"f16 crops, first-step error {err0}: {share:.3f} of the steps set aside")
        assert share <= T.QUARTER
    ref = TorchIcrOracle(make_icr_state(0)).logits(crnn_numpy.normalize_u8(pr.align_collate_pil(T.surface_fragments(), 100)))
    share = _share(ref, 2e-3)
    print(f"processor surface: {share:.3f} of the steps set aside")
    assert share <= T.QUARTER
