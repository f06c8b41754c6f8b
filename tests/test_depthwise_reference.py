"""The instrument of the depthwise tests, proven on the CPU: the direct NumPy statement of tests/depthwise_ref.py equals the dense
references on block-diagonal filters -- tests/exact.conv_truth bit for bit on the lattice, the C oracle within the suite's tolerance on
continuous operands -- every listed lattice case has headroom, and expand / diag are inverses on a whole net."""
import numpy as np
import pytest

from tests import depthwise_ref as D
from tests import exact as X
from tests import util


def _runs():
    return [(c, X.WIDE) for c in D.CASES] + [(c, X.NARROW) for c in D.NARROW_CASES]


@pytest.mark.parametrize("case,lattice", _runs(), ids=lambda v: D.key(v) if len(v) > 2 else "amp%d" % v[0])
def test_direct_statement_equals_the_dense_truth_on_expanded_filters(case, lattice):
    (x, w, b, dy, _), (y, S_gw, S_gb, dx) = D.lattice_case(case, lattice)
    Y, S_GW, S_GB, DX = X.conv_truth(D.dense_case(case), x, D.expand_filters(w), b, dy)
    X.bits_equal(y, Y, "y")
    X.bits_equal(dx, DX, "dx")
    assert np.array_equal(S_gw, D.diag_filters(S_GW)) and np.array_equal(S_gb, S_GB)
    off = S_GW.copy()
    idx = np.arange(case[1])
    off[idx, idx] = 0
    assert case[1] == 1 or np.abs(off).max() > 0  # (the dense sum off the diagonal is not zero: taking the diagonal is a real selection)
    for divisor in (1.0, 3.0, 4.0):
        X.bits_equal(X.divided(S_gw, divisor), D.diag_filters(X.divided(S_GW, divisor)), f"gw / {divisor}", 1.0 / divisor)
        X.bits_equal(X.divided(S_gb, divisor), X.divided(S_GB, divisor), f"gb / {divisor}", 1.0 / divisor)


@pytest.mark.parametrize("case", D.CASES, ids=D.key)
def test_every_lattice_case_has_headroom(case):
    """terms per output: k*k + 1 (forward), k*k (data gradient), B * Ho * Wo (weight gradient)"""
    B, C, H, W, k, s, pad, Ho, Wo = D.geometry(case)
    for amp, bias_amp in (X.WIDE, X.NARROW):
        h = D.headroom(case, amp, bias_amp)
        assert h == max(amp * amp * k * k + bias_amp, amp * amp * B * Ho * Wo) and h < X.LIMIT
    (x, w, b, dy, below), (y, S_gw, S_gb, dx) = D.lattice_case(case)
    assert max(np.abs(y).max(), np.abs(dx).max(), np.abs(S_gw).max(), np.abs(S_gb).max()) <= D.headroom(case)
    assert (below == 0).any() and (below > 0).any()


def test_a_row_no_window_covers_is_zero_in_the_truth():
    case = D.K3_S2[1]  # (2, 4, 10, 13, 3, 2, 0): Ho = 4 covers rows 0..8
    dx = D.lattice_case(case)[1][3]
    assert not dx[:, :, 9].any() and dx[:, :, 8].any()
    assert not np.signbit(dx[:, :, 9]).any()


@pytest.mark.parametrize("case", D.CASES, ids=D.key)
def test_direct_statement_equals_the_c_oracle_on_expanded_filters(case):
    (x, w, b, dy, _), (y, gw, gb, dx) = D.continuous_case(case)
    Y, S_gw, S_gb, DX = D.dw_f64(case, x, w, b, dy)
    util.assert_close(Y, y, what="y")
    util.assert_close(DX, dx, what="dx")
    util.assert_close(S_gw / case[0], gw, what="gw")
    util.assert_close(S_gb / case[0], gb, what="gb")


def test_expand_and_diag_are_inverses_on_a_net():
    from cnn_amd import stacks

    spec = [("conv", 8, 3, 2, 1), ("bn",), ("relu",), ("dwconv", 3, 1, 1), ("bn",), ("relu",), ("conv", 16, 1, 1, 0), ("relu",),
            ("dwconv", 3, 2, 1), ("relu",), ("pool", 2, 2), ("linear", 3)]
    layout = stacks.walk(spec, 3, 33, 29)
    xspec = D.expand_spec(spec)
    assert xspec[3] == ("conv", 8, 3, 1, 1) and xspec[8] == ("conv", 16, 3, 2, 1) and len(xspec) == len(spec)
    xlayout = stacks.walk(xspec, 3, 33, 29)
    assert [e["out"] for e in xlayout] == [e["out"] for e in layout]
    n = sum(e["params"] for e in layout)
    flat = np.arange(1, n + 1, dtype=np.float32)
    big = D.expand_params(layout, flat)
    assert big.size == sum(e["params"] for e in xlayout) == D.expanded_count(layout)
    assert np.array_equal(D.diag_grads(layout, big), flat)
    assert np.count_nonzero(big) == n  # nothing but the originals and zeros
    w = flat[layout[0]["params"] + layout[1]["params"]:][:8 * 9].reshape(8, 1, 3, 3)
    W = D.expand_filters(w)
    assert W.shape == (8, 8, 3, 3) and np.array_equal(W[5, 5], w[5, 0]) and not W[5, 4].any()
