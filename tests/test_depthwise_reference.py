"""The instrument of the depthwise tests, proven on the CPU: the direct NumPy statement of tests/depthwise_ref.py equals the dense
references on block-diagonal filters -- tests/exact.conv_truth bit for bit on the lattice, the C oracle within the suite's tolerance on
continuous operands -- every listed lattice case has headroom, and expand / diag are inverses on a whole net."""
import numpy as np
import pytest

from tests import depthwise_ref as D
from tests import exact as X
from tests import util


def _runs():
    return [(c, X.WIDE) for c in D.CASES] + [(c, X.NARROW) for c in D.NARROW_CASES + D.VARIANT_NARROW_CASES]


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


def _reachable():
    """every (kernel, S, OFF or PP, v) a 3x3 launch can choose: 3 <= W <= 20, pad 0..4, both strides, x / dy / outputs each aligned or
    4 bytes off (relu_below with the outputs: its own shift only removes the float4 body and adds no combination)"""
    out = set()
    for W in range(3, 21):
        for pad in range(5):
            for s in (1, 2):
                for sx in (0, 4):
                    for sdy in (0, 4):
                        for so in (0, 4):
                            out |= D.variants((1, 1, W, W, 3, s, pad), D.shifts_of((sx, sdy, so, so)))
    return out


def _hit(cases, rows):
    return set().union(*(D.variants(c, D.shifts_of(r)) for c in cases for r in rows))


def test_the_gpu_cases_reach_every_load_and_store_variant():
    """the model of conv_depthwise.hip's choice (dw_off, vst, vdy): 34 reachable combinations, all of them launched by the GPU case list
    with its shift rows (tests/test_gpu_depthwise.py compares the model with the tag of every launch); the odd-width cases alone: 9"""
    reachable = _reachable()
    assert len(reachable) == 34
    assert {v[0] for v in reachable} == {"dw_fwd", "dw_dgrad", "dw_wgrad"}
    for kernel in ("dw_fwd", "dw_wgrad"):  # every load instance and both vector flags, at both strides
        assert {(S, off) for k_, S, off, v in reachable if k_ == kernel} == {(S, off) for S in (1, 2) for off in (0, 1, 2, -1)}
    # (the stride-1 data gradient: OFF 0 and 2 mean an even pad' = 2 - pad, so W = Wo + 2 * pad' - 2 is no multiple of 4: scalar stores)
    assert {(off, v) for k_, S, off, v in reachable if (k_, S) == ("dw_dgrad", 1)} == {(0, 0), (2, 0), (1, 0), (1, 1), (-1, 0), (-1, 1)}
    assert {(pp, v) for k_, S, pp, v in reachable if (k_, S) == ("dw_dgrad", 2)} == {(pp, v) for pp in (0, 1) for v in (0, 1)}
    old = _hit(D.ODD_WIDTH_CASES, D.SHIFTS_BOTH)
    assert len(old) == 9 and old < reachable
    assert not any(off >= 0 for k_, S, off, v in old if (k_, S) != ("dw_dgrad", 2))  # no float4 load body at all
    new = _hit(D.VARIANT_CASES, D.SHIFT_ROWS)
    assert new == reachable, sorted(reachable - new)
    assert D.variants(D.GENERIC[0], D.shifts_of(D.SHIFT_ROWS[0])) == set()
    assert set(D.VARIANT_CASES).isdisjoint(D.ODD_WIDTH_CASES) and len(set(D.CASES)) == len(D.CASES)
    assert all(D.dw_off(True, 8, pad) == want for pad, want in ((0, 0), (1, 1), (2, 2), (3, -1), (4, 0), (-1, -1), (-2, 2)))
    assert D.dw_off(False, 8, 1) == -1 and D.dw_off(True, 6, 1) == -1
    assert D.tag_variant("dw_fwd<3x3,s2>|B2 Ci3 8x8 Co3 k3 s2 p1 off-1 v1") == ("dw_fwd", 2, -1, 1)
    assert D.tag_variant("dw_dgrad<3x3,s2>|B2 Ci3 8x8 Co3 k3 s2 p1 pp1 v0") == ("dw_dgrad", 2, 1, 0)
    assert D.tag_variant("dw_dgrad<3x3,s2>|B2 Ci3 8x8 Co3 k3 s2 p1 off1 v0") is None
    assert D.tag_variant("dw_fwd<3x3,s2>|B2 Ci3 8x8 Co3 k3 s2 p1") is None


def test_padding_wider_than_the_filter_reach_is_the_bias_in_the_truth():
    """pad = 3: the outermost output rows and columns see nothing but padding and equal the bias; dx is cropped back and still non-zero"""
    case = D.VARIANT_S1[7]  # (1, 2, 5, 8, 3, 1, 3)
    assert case[6] == 3
    (x, w, b, dy, _), (y, S_gw, S_gb, dx) = D.lattice_case(case)
    for border in (y[:, :, 0], y[:, :, -1], y[:, :, :, 0], y[:, :, :, -1]):
        assert np.array_equal(border, np.broadcast_to(b[None, :, None], border.shape))
    assert not np.array_equal(y[:, :, 1], np.broadcast_to(b[None, :, None], y[:, :, 1].shape))  # (the next row in does see the input)
    assert dx.shape == x.shape and dx.any() and all(dx[:, :, i].any() for i in (0, -1)) and all(dx[:, :, :, j].any() for j in (0, -1))


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
