"""The instrument behind tests/test_gpu_exact_sums.py, proven without a device (tests/exact.py): on lattice operands the fp32 C oracle,
in the reference's own loop order, equals the integer restatement bit for bit; every desc used on the GPU stays below 2^24; the inputs
hold the zeros and ties the GPU comparisons rely on; and a single missing product of magnitude 1 fails bits_equal where the 1e-4
tolerance may let it pass.

The oracle agreement runs over every desc of conv_route_cases.HAND_PICKED (none left out: the threaded C oracle needs about a second
for the largest, the 112-wide north-star desc, and less than half of one for any other), the 1x1 descs of exact.C11_CASES and the
linear shapes of test_linear_vs_oracle.  The oracle divides the weight gradient per sample and accumulates, so its gw / gb equal
sum / B only where B is a power of two: compared there."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import conv_route_cases as R
from tests import exact as X
from tests.util import REL_TOL, rel_err

ALL_CONV = list(dict.fromkeys(tuple(c[:8]) for c in R.HAND_PICKED)) + X.C11_CASES
LATTICES = [X.WIDE, X.NARROW]
_id = lambda c: R.key(c)
_lat = lambda l: "amp%d" % l[0]


@pytest.mark.parametrize("lattice", LATTICES, ids=_lat)
@pytest.mark.parametrize("case", ALL_CONV, ids=_id)
def test_c_oracle_equals_the_integer_truth(case, lattice):
    (x, w, b, dy), (y, S_gw, S_gb, dx) = X.lattice_conv(case, X.seed_of(case, lattice[0]), *lattice)
    B, pad, s = case[0], case[7], case[6]
    X.bits_equal(O.conv2d_forward_padded(x, w, b, s, pad), y, "oracle y")
    gw, gb, odx = O.conv2d_backward_padded(x, dy, w, s, pad)
    X.bits_equal(odx, dx, "oracle dx")
    if B & (B - 1) == 0:
        X.bits_equal(gw, X.divided(S_gw, B), "oracle gw", 1.0 / B)
        X.bits_equal(gb, X.divided(S_gb, B), "oracle gb", 1.0 / B)


def test_per_sample_division_is_not_the_quotient_of_the_sum():
    """why the reference for gw / gb is the integer restatement where the divisor is no power of two: the oracle (like the reference)
    divides every sample's contribution and accumulates the rounded quotients"""
    case = (3, 32, 9, 11, 64, 3, 1, 0)
    (x, w, b, dy), (_, S_gw, _, _) = X.lattice_conv(case, X.seed_of(case), *X.WIDE)
    gw, _, _ = O.conv2d_backward_padded(x, dy, w, 1, 0, need=(True, True, False))
    assert X.bits_differ(gw, X.divided(S_gw, 3.0), "oracle gw at B = 3") is not None
    assert rel_err(gw, X.divided(S_gw, 3.0)) < 1e-6


@pytest.mark.parametrize("lattice", LATTICES, ids=_lat)
@pytest.mark.parametrize("shape", X.LINEAR_SHAPES, ids=lambda s: "B%d_%d_%d" % s)
def test_c_oracle_linear_equals_the_integer_truth(shape, lattice):
    B = shape[0]
    x, w, b, dy = X.linear_inputs(*shape, 31, *lattice)
    y, S_gw, S_gb, dx = X.linear_truth(x, w, b, dy)
    X.bits_equal(O.linear_forward(x, w, b), y, "oracle linear y")
    gw, gb, odx = O.linear_backward(x, dy, w)
    X.bits_equal(odx, dx, "oracle linear dx")
    if B & (B - 1) == 0:
        X.bits_equal(gw, X.divided(S_gw, B), "oracle linear gW", 1.0 / B)
        X.bits_equal(gb, X.divided(S_gb, B), "oracle linear gb", 1.0 / B)


@pytest.mark.parametrize("lattice", LATTICES, ids=_lat)
def test_headroom_of_every_desc_used_on_the_gpu(lattice):
    from tests.test_gpu_parity import CONV_CASES  # (the im2col entries run on the descs of test_conv2d_im2col_fallback_vs_oracle)

    for c in ALL_CONV + CONV_CASES:
        assert X.headroom(c, *lattice) < X.LIMIT, c
    for s in X.LINEAR_SHAPES:
        assert X.linear_headroom(*s, *lattice) < X.LIMIT, s
    for B, H, W in X.FIRST_BLOCK_SHAPES:
        c = (B, 3, H, W, 16, 3, 2, 0)
        Ho, Wo = X.geometry(c)[8:]
        assert X.headroom(c, *X.NARROW, dy_amp=8, dy_terms=B * (Ho // 2) * (Wo // 2)) < X.LIMIT, c
    assert X.headroom((256, 64, 112, 112, 128, 3, 1, 0), *X.WIDE) >= X.LIMIT  # (the bound is not vacuous: a full batch leaves the lattice)


@pytest.mark.parametrize("shape", X.FIRST_BLOCK_SHAPES, ids=lambda s: "B%d_%dx%d" % s)
def test_first_block_inputs_hold_zero_windows_and_tied_maxima(shape):
    """from the truth alone: at least 2 % all-zero windows and 2 % windows whose positive maximum sits at two window positions where
    there are 500 windows or more, at least one of each below that"""
    B, H, W = shape
    case = (B, 3, H, W, 16, 3, 2, 0)
    t = X.first_block_truth(case, X.seed_of(case, 1))
    n, zero, tied = X.window_shares(t["relu"])
    assert n == t["pooled"].size
    if n >= 500:
        assert zero >= 0.02 * n and tied >= 0.02 * n, (n, zero, tied)
    else:
        assert zero >= 1 and tied >= 1, (n, zero, tied)
    assert int(t["dead"].sum()) == zero
    # the routed gradient reaches tied windows: some live window with a tie has a non-zero dpool
    assert np.count_nonzero(t["dy"]) > 0


@pytest.mark.parametrize("lattice", LATTICES, ids=_lat)
@pytest.mark.parametrize("case", ALL_CONV, ids=_id)
def test_inputs_hold_exact_zeros_at_both_relu_decisions(case, lattice):
    """every desc runs forward_relu and backward_data_relu: at least one y == 0 out of the accumulator, and at least one relu_below == 0
    above a non-zero unmasked dx"""
    (x, w, b, dy), (y, _, _, dx) = X.lattice_conv(case, X.seed_of(case, lattice[0]), *lattice)
    assert np.count_nonzero(y == 0) >= 1, "no y == 0: choose another seed in tests/exact.py"
    assert np.count_nonzero((np.maximum(x, 0) == 0) & (dx != 0)) >= 1


def _drop_one_product(t):
    """t with one product of magnitude 1 removed from its largest element"""
    out = t.copy()
    i = np.unravel_index(np.argmax(np.abs(t)), t.shape)
    out[i] -= np.sign(t[i])
    return out


def test_one_missing_unit_product_fails_bits_equal_where_the_tolerance_may_not():
    """A product of magnitude 1 (the smallest the wide lattice has; the largest is 64) missing from one element moves the tensor-normalised
    error by 1 / max|t|: below REL_TOL where max|t| > 10^4, and only there.  Measured on these operands: max|y| = 2739 for the north-star
    forward sums (576 terms; ratio 3.65e-4) and 8903 for the 25088-input linear layer's logits (1.12e-4): both above REL_TOL, so the
    tolerance does see them; max|S| = 10749 for the first layer's weight-gradient sums at 224 x 224 (24642 terms; 9.30e-5), which the
    tolerance lets pass.  bits_equal sees all three.  The claim is only that: the exact comparison sees what the tolerance may not."""
    north = (1, 64, 112, 112, 128, 3, 1, 0)
    first = (2, 3, 224, 224, 16, 3, 2, 0)
    lin = X.linear_inputs(19, 25088, 3, 31)
    tensors = {"north-star y": X.lattice_conv(north, X.seed_of(north), *X.WIDE)[1][0],
               "linear 25088 y": X.linear_truth(*lin)[0],
               "first layer S_gw": X.lattice_conv(first, X.seed_of(first), *X.WIDE)[1][1].astype(np.float32)}
    hidden = 0
    for name, t in tensors.items():
        bad = _drop_one_product(t)
        top = float(np.abs(t).max())
        e = rel_err(bad, t)
        print(f"{name}: max|t| = {top:.0f}, one unit product = {e:.2e} of it")
        report = X.bits_differ(bad, t, name)
        assert report and ("difference -1 lattice" in report or "difference +1 lattice" in report), report
        assert (e <= REL_TOL) == (top >= 1e4), (name, top, e)
        hidden += e <= REL_TOL
    assert hidden >= 1
