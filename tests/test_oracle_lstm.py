"""CPU checks of oracle/lstm_ref.py, the fp64 reference, bound and operand sets of tests/test_lstm_gpu.py: the reference is
torch.nn.LSTM, the operand sets carry the teeth they claim, a numpy emulation of the kernels' arithmetic stays inside the bound
at every case of the GPU table, and the same emulation with any one of six kernel bugs breaks the bound by at least ten times —
so a kernel with one of these bugs cannot pass that test.

Measured here, max over elements of err / bound, lowest .. highest of the four mutation cases (f16 | fp32), libm's exp2 in the
place of v_exp_f32.  The largest ratios sit where h is close to 0 and the bound with it:
    clean emulation, worst case of the table            0.97 | 0.34     (f16: the half-ulp rounding of h, which the bound meets)
    zero_fragment                             2.9e3 .. 4.4e3 | 4.1e3 .. 1.2e4
    swap_units                                1.2e4 .. 2.3e5 | 2.5e4 .. 3.5e5
    stale_h                                   7.5e3 .. 4.2e4 | 1.7e4 .. 1.0e5
    reverse_walks_forward                     2.9e6 .. 6.7e6 | 3.7e6 .. 1.2e7
    swap_f_i                                  2.5e6 .. 2.7e6 | 2.9e6 .. 3.1e6
    scale_c by 1 - 1e-2                          61 .. 155   | 197 .. 403
"""
import numpy as np
import pytest

from oracle import lstm_ref as R

PARAMS = R.case_params()
MUTATION_CASES = [(p, kw) for p, kw in PARAMS if kw["T"] >= 24 and not kw["saturated"]]     # a bug in the recurrence needs a history


def _ratio(whh, xproj, f16, mutation=None):
    dev = R.emulate(whh, xproj, f16, mutation)
    ref = R.reference_forced(R.rounded(whh, f16), xproj, dev, f16)
    return float((np.abs(dev - ref["h"]) / ref["bound"]).max()), dev, ref


@pytest.mark.parametrize("T", [1, 2, 7])
def test_reference_is_torch_lstm(T):
    """gate order i, f, g, o and the reverse direction's indexing, against the operation's definition"""
    import torch

    torch.manual_seed(T)
    B, IN = 3, 8
    m = torch.nn.LSTM(IN, R.HID, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-0.3, 0.3)
    x = torch.randn(B, T, IN, dtype=torch.float64)
    with torch.no_grad():
        want = m(x)[0].numpy()
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    whh = np.stack([sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]])
    xproj = np.stack([x.numpy() @ sd["weight_ih_l0" + r].T + sd["bias_ih_l0" + r] + sd["bias_hh_l0" + r] for r in ("", "_reverse")], axis=2)
    assert xproj.shape == (B, T, 2, 4 * R.HID)
    got = R.reference_free(whh, xproj)
    assert np.abs(got - want).max() <= 1e-12
    # teacher-forced on its own output, the forced form is the same function
    forced = R.reference_forced(whh, xproj, got, f16=False)
    assert np.abs(forced["h"] - want).max() <= 1e-12


def test_operand_sets_have_their_teeth():
    whh, x = R.make_case(33, 63, 1)
    assert whh.shape == (2, 1024, 256) and x.shape == (33, 63, 2, 1024)
    assert np.abs(whh).max() <= np.sqrt(3 / 256) and np.abs(R.make_case(33, 63, 3)[0]).max() > 2 * np.sqrt(3 / 256)
    sat = np.abs(x) == 40
    for gate in range(4):       # both signs of a saturated column in every gate, in one row and step
        g = x[0, 0, 0, gate * 256:(gate + 1) * 256]
        assert (g == 40).any() and (g == -40).any()
    assert sat[:, :, :, 37].all() and not sat[:, :, :, 38].any()
    ref = R.reference_forced(whh, x, R.reference_free(whh, x), f16=False)
    assert ref["c_max"] >= 0.95 * 63                     # |c| climbs to about T: past the overflow of exp2 inside tanh(c)
    pre_max = 2 * R.L2E * ref["c_max"]
    assert pre_max > 128
    whh, x = R.make_case(16, 63, 3, saturated=True)
    assert (np.abs(x) == 40).all() and (x > 0).any() and (x < 0).any()


def test_saturation_limits_of_the_emulated_gates():
    """exp2 -> inf -> 1 / inf -> 0: the limits are exact, never NaN"""
    big = np.array([-1e30, -200.0, -89.0, -45.0, 45.0, 89.0, 200.0, 1e30], np.float32)
    assert (R._fast_sigmoid(big) == np.array([0, 0, 0, R._fast_sigmoid(np.float32(-45)), 1, 1, 1, 1], np.float32)).all()
    assert (R._fast_tanh(big) == np.array([-1, -1, -1, -1, 1, 1, 1, 1], np.float32)).all()


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("pid,kw", PARAMS, ids=[p for p, _ in PARAMS])
def test_clean_emulation_is_within_the_bound(pid, kw, f16):
    whh, x = R.make_case(**kw)
    ratio, dev, ref = _ratio(whh, x, f16)
    print(f"{pid} {'f16' if f16 else 'f32'}: clean max err / bound {ratio:.3f}")
    assert np.isfinite(dev).all() and np.isfinite(ref["bound"]).all()
    assert ratio <= 1.0, (pid, ratio)
    err = np.abs(dev - ref["h"])
    assert err.mean() <= ref["mean_bound"].mean()


@pytest.mark.parametrize("mutation", R.MUTATIONS)
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("pid,kw", MUTATION_CASES, ids=[p for p, _ in MUTATION_CASES])
def test_each_kernel_bug_breaks_the_bound(pid, kw, f16, mutation):
    whh, x = R.make_case(**kw)
    ratio, _, _ = _ratio(whh, x, f16, mutation)
    print(f"{pid} {'f16' if f16 else 'f32'}: {mutation} max err / bound {ratio:.3g}")
    assert ratio >= 10.0, (pid, mutation, ratio)


def test_table_covers_the_shapes_the_kernels_branch_on():
    shapes = {(B, T) for B, T, _, _ in R.GPU_CASES}
    assert {(1, 1), (15, 2), (16, 3), (17, 24), (33, 63), (16, 63)} == shapes
    assert len(MUTATION_CASES) == 4
