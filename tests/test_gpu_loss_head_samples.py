"""The loss head with several samples per workgroup (linear_fwd_softmax_xent<.., S>, CNN_AMD_HEAD_SAMPLES = 1 | 2 | 4 | 8) against the
unfused trio cnn_linear_forward_softmax_xent + cnn_linear_backward[_relu]: logits, probabilities, delta, loss terms and dx bit for
bit, for every S the library builds.

B = 1, 2, 3, 4, 5, 7, 9: a lone tail workgroup, a full workgroup plus every tail length for S = 2 and 4, more than two workgroups.
in = 4608 (x and W stay in registers for the dx pass), 9216 (the 18-wide loop twice: nothing is kept), 7000 (ragged: the 18-wide loop
once, the 4-wide loop twice, then one or two leftover elements per thread).  Every output buffer has two guard rows behind sample B - 1 that must keep
their sentinel: a workgroup at the batch's tail writes nothing at a sample index >= B.
"""
import numpy as np
import pytest

from tests.util import normal_scaled, uniform_pm1

pytestmark = pytest.mark.gpu

SAMPLES = (1, 2, 4, 8)
BATCHES = (1, 2, 3, 4, 5, 7, 9)
WIDTHS = (4608, 9216, 7000)
GUARD = 2
SENTINEL = -123.25
NAMES = ("logits", "probs", "delta", "loss terms", "dx")


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    arch = capi.load().cnn_amd_device_arch().decode()
    assert arch == "gfx950", f"built for gfx950, running on {arch}"
    return torch


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def trio(T, x, w, b, labels, relu):
    """the reference: the forward + loss kernel (always one sample per workgroup, whatever the option says) and the separate
    backward kernel"""
    from cnn_amd import capi

    lib, P = capi.load(), capi._ptr
    B, n_in = x.shape
    mk = lambda *shape: T.full(shape, SENTINEL, device="cuda")
    logits, probs, delta, terms = mk(B, 3), mk(B, 3), mk(B, 3), mk(B)
    capi.check(lib.cnn_linear_forward_softmax_xent(P(x), P(w), P(b), P(labels), P(logits), P(probs), P(delta), P(terms), B, n_in, 3,
                                                   capi._stream()), "cnn_linear_forward_softmax_xent")
    _, _, dx = capi.linear_backward(x, delta, w, float(B), relu_below=bool(relu))
    return [u32(t) for t in (logits, probs, delta, terms, dx)]


def fused(T, x, w, b, labels, relu, S):
    """the one-kernel head with S samples per workgroup; asserts that the guard rows behind sample B - 1 are untouched"""
    from cnn_amd import capi

    lib, P = capi.load(), capi._ptr
    B, n_in = x.shape
    mk = lambda *shape: T.full(shape, SENTINEL, device="cuda")
    logits, probs, delta, terms, dx = mk(B + GUARD, 3), mk(B + GUARD, 3), mk(B + GUARD, 3), mk(B + GUARD), mk(B + GUARD, n_in)
    with capi.option("HEAD_SAMPLES", S):
        capi.check(lib.cnn_linear_forward_softmax_xent_dx(P(x), P(w), P(b), P(labels), P(logits), P(probs), P(delta), P(terms), P(dx),
                                                          int(relu), B, n_in, 3, capi._stream()), "cnn_linear_forward_softmax_xent_dx")
    T.cuda.synchronize()
    sentinel = np.float32(SENTINEL).view(np.uint32)
    out = []
    for name, t in zip(NAMES, (logits, probs, delta, terms, dx)):
        a = u32(t)
        assert np.all(a[B:] == sentinel), (name, "guard rows", S, B, n_in)
        out.append(a[:B])
    return out


_reference = {}


def case(T, B, n_in, relu):
    """inputs and the trio's results of one shape: computed once, shared by every S"""
    key = (B, n_in, relu)
    if key not in _reference:
        xh = uniform_pm1(900 + B, (B, n_in))
        if relu:
            xh = np.maximum(xh, 0)  # a ReLU layer's output: zeros where its backward mask applies
        x, w, b = dev(T, xh), dev(T, normal_scaled(901, (n_in, 3))), dev(T, normal_scaled(902, (3,)))
        labels = dev(T, ((np.arange(B) + 1) % 3).astype(np.int32))
        _reference[key] = (x, w, b, labels, trio(T, x, w, b, labels, relu))
    return _reference[key]


@pytest.mark.parametrize("relu", [0, 1], ids=["plain", "relu_below"])
@pytest.mark.parametrize("S", SAMPLES)
def test_head_with_S_samples_per_workgroup_is_bit_identical(T, S, relu):
    for n_in in WIDTHS:
        for B in BATCHES:
            x, w, b, labels, ref = case(T, B, n_in, relu)
            got = fused(T, x, w, b, labels, relu, S)
            for name, a, c in zip(NAMES, ref, got):
                assert np.array_equal(a, c), (name, S, B, n_in)


def test_a_sample_count_without_a_kernel_is_refused(T):
    from cnn_amd import capi

    x, w, b, labels, _ = case(T, 2, 4608, 0)
    with pytest.raises(capi.CnnAmdError):
        fused(T, x, w, b, labels, 0, 3)


@pytest.fixture(scope="module")
def edge(T):
    """4608 -> 3, B = 9 (samples 0..3 share a workgroup at S = 4, all but the last at S = 8):
    sample 0: +0 and -0 among the x values (the ReLU mask x <= 0 holds for both), negative values beside them;
    sample 1: logits more than 88 apart: the clamped exponential returns 0 for the small one, whose log(0) * 0 makes the loss term NaN;
    sample 2: the same the other way round;
    sample 3: one NaN x value -- in `x_nan` only; `x` has a finite value there"""
    B, n_in = 9, 4608
    xh = uniform_pm1(950, (B, n_in))
    wh, bh = normal_scaled(951, (n_in, 3)), normal_scaled(952, (3,))
    xh[0, 0:512:2] = 0.0
    xh[0, 1:512:4] = -0.0
    d = wh[:, 0].astype(np.float64) - wh[:, 1]
    xh[1] = (np.sign(d) * 200.0 / np.abs(d).sum()).astype(np.float32)
    xh[2] = -xh[1]
    labels = ((np.arange(B) + 1) % 3).astype(np.int32)
    xn = xh.copy()
    xn[3, 17] = np.nan
    x, x_nan, w, b, lab = dev(T, xh), dev(T, xn), dev(T, wh), dev(T, bh), dev(T, labels)
    refs = {(nan, relu): trio(T, x_nan if nan else x, w, b, lab, relu) for nan in (0, 1) for relu in (0, 1)}
    logits = refs[(0, 0)][0].view(np.float32)
    assert logits[1].max() - logits[1].min() > 88 and logits[2].max() - logits[2].min() > 88
    assert np.any(refs[(0, 0)][1].view(np.float32)[1:3] == 0)  # (a probability of exactly 0: the clamp was hit)
    return x, x_nan, w, b, lab, refs


@pytest.mark.parametrize("relu", [0, 1], ids=["plain", "relu_below"])
@pytest.mark.parametrize("S", SAMPLES)
def test_head_edge_values_with_S_samples_per_workgroup(T, edge, S, relu):
    x, x_nan, w, b, labels, refs = edge
    got = fused(T, x, w, b, labels, relu, S)
    for name, a, c in zip(NAMES, refs[(0, relu)], got):
        assert np.array_equal(a, c), (name, S)
    if relu:  # the mask took +0 and -0 alike
        assert np.all(got[4][0, 0:512:2] == 0) and np.all(got[4][0, 1:512:4] == 0)
    got_nan = fused(T, x_nan, w, b, labels, relu, S)
    for name, a, c, clean in zip(NAMES, refs[(1, relu)], got_nan, got):
        assert np.array_equal(a, c), (name, S, "the NaN sample's row against the trio")
        others = np.arange(a.shape[0]) != 3
        assert np.array_equal(c[others], clean[others]), (name, S, "a NaN in sample 3 reached another sample")
    assert np.all(np.isnan(got_nan[0].view(np.float32)[3]))
