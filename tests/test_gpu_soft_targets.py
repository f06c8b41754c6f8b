"""The soft-target kernels on the device: cnn_soft_targets and cnn_batch_mix bit for bit against the NumPy restatement
(tests/soft_target_ref.py), and the soft loss entries (cnn_softmax_xent_soft, cnn_linear_forward_softmax_xent_soft[_dx]) against their
hard-label counterparts on one-hot targets (bit for bit in logits, probs, delta, loss terms and dx) and on real soft targets."""
import ctypes

import numpy as np
import pytest

from tests.soft_target_ref import (MIX_CUTMIX, MIX_MIXUP, PAIR_FLIP, PAIR_NONE, PAIR_ROLL, ref_batch_mix, ref_soft_targets)
from tests.util import normal_scaled, uniform_pm1

pytestmark = pytest.mark.gpu

SAMPLES = (1, 2, 4, 8)
BATCHES = (1, 2, 3, 4, 5, 7, 9)
WIDTHS = (4608, 9216, 7000)
GUARD = 2
SENTINEL = -123.25
NAMES = ("logits", "probs", "delta", "loss terms", "dx")
EPS32 = 2.0 ** -24


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


SENT_BITS = np.float32(SENTINEL).view(np.uint32)


# ---- cnn_soft_targets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [3, 8, 10])
def test_soft_targets_equal_the_restatement(T, classes):
    """B = 1, 2, 5, 7; NONE, FLIP, ROLL by 1 and by B - 1; smoothing 0 and 0.1; lam 1, 0 and 0.3; one label of -1 and one equal to
    `classes`; two guard rows behind row B - 1 keep their sentinel"""
    from cnn_amd import capi

    for B in (1, 2, 5, 7):
        labels = (np.arange(B) * 2 + 1) % classes
        if B >= 5:
            labels[1], labels[3] = -1, classes
        labels = labels.astype(np.int32)
        ld = dev(T, labels)
        rules = [(PAIR_NONE, 0), (PAIR_FLIP, 0)] + ([(PAIR_ROLL, 1), (PAIR_ROLL, B - 1)] if B > 1 else [])
        for rule, shift in rules:
            for smoothing in (0.0, 0.1):
                for lam in (1.0, 0.0, 0.3):
                    out = T.full((B + GUARD, classes), SENTINEL, device="cuda")
                    capi.soft_targets(ld, classes, smoothing, lam, rule, shift, out=out)
                    got = u32(out)
                    want = ref_soft_targets(labels, classes, smoothing, lam, rule, shift).view(np.uint32)
                    assert np.array_equal(got[:B], want), (B, rule, shift, smoothing, lam)
                    assert np.all(got[B:] == SENT_BITS), ("guard rows", B, rule, shift)


# ---- cnn_batch_mix ------------------------------------------------------------------------------------------------------------------
MIX_SHAPES = [(5, 3, 7, 9), (4, 3, 8, 8), (3, 1, 1, 1), (6, 3, 64, 68)]
SPECIALS = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC01234, 0xFFC00001, 0x00000001, 0x807FFFFF, 0x00400000], np.uint32)


def _mix_input(shape, seed):
    x = uniform_pm1(seed, shape)
    flat = x.reshape(shape[0], -1).view(np.uint32)
    n = min(len(SPECIALS), flat.shape[1])
    flat[shape[0] // 2, :n] = SPECIALS[:n]  # -0.0, +-inf, NaNs with payloads, denormals (the middle sample: FLIP pairs it with itself at odd B)
    return x


def _run_mix(T, capi, x, so, do, mode, lam, rule, shift, box):
    """src / dst at offsets so / do floats from a 16-byte aligned base; returns dst's words, checks src and dst's guard"""
    n = x.size
    src = T.zeros(n + 8, device="cuda")
    src[so:so + n] = dev(T, x.reshape(-1))
    dst = T.full((n + 8,), SENTINEL, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    y0, y1, x0, x1 = box
    d = capi.MixDesc(mode, lam, rule, shift, y0, y1, x0, x1)
    B, Cc, H, W = x.shape
    capi.check(capi.load().cnn_batch_mix(ctypes.byref(d), capi._ptr(src[so:]), capi._ptr(dst[do:]), B, Cc, H, W, capi._stream()), "cnn_batch_mix")
    T.cuda.synchronize()
    assert np.array_equal(u32(src[so:so + n]), x.reshape(-1).view(np.uint32)), "src changed"
    g = u32(dst)
    assert np.all(g[:do] == SENT_BITS) and np.all(g[do + n:] == SENT_BITS), "guard elements around dst"
    return g[do:do + n].reshape(x.shape)


@pytest.mark.parametrize("shape", MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_mix_equals_the_restatement(T, shape):
    from cnn_amd import capi

    B, Cc, H, W = shape
    x = _mix_input(shape, 40 + B)
    rules = [(PAIR_FLIP, 0)] + ([(PAIR_ROLL, 1), (PAIR_ROLL, B - 1)] if B > 1 else [])
    boxes = [(0, H, 0, W), (1 if H > 1 else 0,) * 2 + (0, W), (0, 1, 0, 1), (0, 1, W - 1, W), (H - 1, H, 0, 1), (H - 1, H, W - 1, W)]
    if W >= 8 and H >= 4:
        boxes += [(1, H - 1, 3, 6), (0, 3, 5, W)]  # odd x0 and a width that is no multiple of 4; a box that ends at the right edge
    cases = [(MIX_MIXUP, lam, r, s, (0, 0, 0, 0)) for lam in (0.0, 0.3, 1.0) for r, s in rules]
    cases += [(MIX_CUTMIX, 0.5, r, s, box) for box in boxes for r, s in rules[:2]]
    cases += [(MIX_MIXUP, 0.3, PAIR_NONE, 0, (0, 0, 0, 0)), (MIX_CUTMIX, 0.5, PAIR_NONE, 0, boxes[0])]
    for so in (0, 1):
        for do in (0, 1):
            for mode, lam, rule, shift, box in cases:
                got = _run_mix(T, capi, x, so, do, mode, lam, rule, shift, box)
                want = ref_batch_mix(x, mode, lam, rule, shift, box).view(np.uint32)
                copies = mode == MIX_CUTMIX or lam == 1.0 or rule == PAIR_NONE
                if not copies:
                    # arithmetic on the special words: where the restatement's result is a NaN the device's must be one too -- which
                    # NaN an operation returns (sign, payload) is the implementation's choice in IEEE 754 -- every other word is compared
                    nan = np.isnan(want.view(np.float32))
                    assert np.array_equal(np.isnan(got.view(np.float32)), nan), (shape, so, do, mode, lam, rule, shift)
                    got, want = np.where(nan, 0, got), np.where(nan, 0, want)
                assert np.array_equal(got, want), (shape, so, do, mode, lam, rule, shift, box, int((got != want).sum()))
                if rule == PAIR_NONE or (mode == MIX_MIXUP and lam == 1.0) or (mode == MIX_CUTMIX and box[0] == box[1]):
                    n = min(len(SPECIALS), Cc * H * W)  # nothing is mixed: the special words are where they were, unchanged
                    assert np.array_equal(got.reshape(B, -1)[B // 2, :n], SPECIALS[:n])


def test_batch_mix_kernel_choice(T):
    """one launch per call, its name begins with bmix_: the float4 kernel when both pointers are aligned and C*H*W % 4 == 0, the scalar
    kernel otherwise, the copy kernels where nothing is mixed"""
    from cnn_amd import capi

    def names(x, so, do, *args):
        T.cuda.synchronize()
        capi.kernel_timing(1)
        _run_mix(T, capi, x, so, do, *args)
        rep = capi.kernel_timing_report()
        capi.kernel_timing(0)
        return {k.split("|")[0]: c for k, (c, _) in rep.items() if k.startswith("bmix_")}

    even, odd = _mix_input((4, 3, 8, 8), 1), _mix_input((5, 3, 7, 9), 2)
    box = (1, 5, 2, 7)
    assert names(even, 0, 0, MIX_MIXUP, 0.3, PAIR_FLIP, 0, box) == {"bmix_mixup_vec": 1}
    assert names(even, 1, 0, MIX_MIXUP, 0.3, PAIR_FLIP, 0, box) == {"bmix_mixup_scalar": 1}
    assert names(odd, 0, 0, MIX_MIXUP, 0.3, PAIR_FLIP, 0, box) == {"bmix_mixup_scalar": 1}
    assert names(even, 0, 0, MIX_CUTMIX, 0.3, PAIR_ROLL, 1, box) == {"bmix_cutmix_vec": 1}
    assert names(odd, 0, 0, MIX_CUTMIX, 0.3, PAIR_ROLL, 1, box) == {"bmix_cutmix_scalar": 1}
    assert names(even, 0, 0, MIX_MIXUP, 1.0, PAIR_FLIP, 0, box) == {"bmix_copy_vec": 1}
    assert names(odd, 0, 1, MIX_CUTMIX, 0.3, PAIR_NONE, 0, box) == {"bmix_copy_scalar": 1}


# ---- the soft loss head --------------------------------------------------------------------------------------------------------------
def hard_head(T, x, w, b, labels, relu, S, out=3):
    """cnn_linear_forward_softmax_xent_dx with S samples per workgroup"""
    from cnn_amd import capi

    lib, P = capi.load(), capi._ptr
    B, n_in = x.shape
    mk = lambda *shape: T.full(shape, SENTINEL, device="cuda")
    bufs = mk(B, out), mk(B, out), mk(B, out), mk(B), mk(B, n_in)
    with capi.option("HEAD_SAMPLES", S):
        capi.check(lib.cnn_linear_forward_softmax_xent_dx(P(x), P(w), P(b), P(labels), *[P(t) for t in bufs], int(relu), B, n_in, out,
                                                          capi._stream()), "cnn_linear_forward_softmax_xent_dx")
    return [u32(t) for t in bufs]


def soft_head(T, x, w, b, targets, relu, S, out=3):
    """cnn_linear_forward_softmax_xent_soft_dx; asserts that the guard rows behind sample B - 1 are untouched"""
    from cnn_amd import capi

    lib, P = capi.load(), capi._ptr
    B, n_in = x.shape
    mk = lambda *shape: T.full(shape, SENTINEL, device="cuda")
    bufs = mk(B + GUARD, out), mk(B + GUARD, out), mk(B + GUARD, out), mk(B + GUARD), mk(B + GUARD, n_in)
    with capi.option("HEAD_SAMPLES", S):
        capi.check(lib.cnn_linear_forward_softmax_xent_soft_dx(P(x), P(w), P(b), P(targets), *[P(t) for t in bufs], int(relu), B, n_in, out,
                                                               capi._stream()), "cnn_linear_forward_softmax_xent_soft_dx")
    T.cuda.synchronize()
    res = []
    for name, t in zip(NAMES, bufs):
        a = u32(t)
        assert np.all(a[B:] == SENT_BITS), (name, "guard rows", S, B, n_in)
        res.append(a[:B])
    return res


_inputs = {}


def case(T, B, n_in, relu, out=3):
    key = (B, n_in, relu, out)
    if key not in _inputs:
        xh = uniform_pm1(900 + B, (B, n_in))
        if relu:
            xh = np.maximum(xh, 0)
        labels = ((np.arange(B) + 1) % out).astype(np.int32)
        _inputs[key] = (dev(T, xh), dev(T, normal_scaled(901, (n_in, out))), dev(T, normal_scaled(902, (out,))), dev(T, labels), labels)
    return _inputs[key]


@pytest.mark.parametrize("relu", [0, 1], ids=["plain", "relu_below"])
@pytest.mark.parametrize("S", SAMPLES)
def test_soft_head_on_one_hot_targets_is_the_hard_head(T, S, relu):
    for n_in in WIDTHS:
        for B in BATCHES:
            x, w, b, ld, labels = case(T, B, n_in, relu)
            onehot = dev(T, np.eye(3, dtype=np.float32)[labels])
            ref = hard_head(T, x, w, b, ld, relu, S)
            got = soft_head(T, x, w, b, onehot, relu, S)
            for name, a, c in zip(NAMES, ref, got):
                assert np.array_equal(a, c), (name, S, B, n_in)


@pytest.fixture(scope="module")
def edge(T):
    """the edge fixture of tests/test_gpu_loss_head_samples.py, rebuilt: 4608 -> 3, B = 9; sample 0: +0 and -0 among the x values;
    samples 1 and 2: logits more than 88 apart (the clamped exponential returns 0, log(0) * 0 makes the loss term NaN); sample 3: one NaN
    x value in `x_nan` only"""
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
    return dev(T, xh), dev(T, xn), dev(T, wh), dev(T, bh), dev(T, labels), dev(T, np.eye(3, dtype=np.float32)[labels])


@pytest.mark.parametrize("relu", [0, 1], ids=["plain", "relu_below"])
@pytest.mark.parametrize("S", SAMPLES)
def test_soft_head_edge_values(T, edge, S, relu):
    x, x_nan, w, b, ld, onehot = edge
    ref, got = hard_head(T, x, w, b, ld, relu, S), soft_head(T, x, w, b, onehot, relu, S)
    for name, a, c in zip(NAMES, ref, got):
        assert np.array_equal(a, c), (name, S)
    logits, probs, terms = got[0].view(np.float32), got[1].view(np.float32), got[3].view(np.float32)
    assert logits[1].max() - logits[1].min() > 88 and np.any(probs[1:3] == 0) and np.any(np.isnan(terms[1:3]))
    ref_nan, got_nan = hard_head(T, x_nan, w, b, ld, relu, S), soft_head(T, x_nan, w, b, onehot, relu, S)
    for name, a, c, clean in zip(NAMES, ref_nan, got_nan, got):
        assert np.array_equal(a, c), (name, S, "the NaN sample's row against the hard head")
        others = np.arange(a.shape[0]) != 3
        assert np.array_equal(c[others], clean[others]), (name, S, "a NaN in sample 3 reached another sample")
    assert np.all(np.isnan(got_nan[0].view(np.float32)[3]))


@pytest.mark.parametrize("out", [3, 10])
def test_generic_soft_entries_on_one_hot_targets(T, out):
    """cnn_linear_forward_softmax_xent_soft (out = 3) and cnn_softmax_xent_soft (3 and 10 classes) against their hard counterparts"""
    from cnn_amd import capi

    lib, P = capi.load(), capi._ptr
    B, n_in = 7, 7000
    x, w, b, ld, labels = case(T, B, n_in, 0, out)
    onehot = dev(T, np.eye(out, dtype=np.float32)[labels])
    logits = capi.linear_forward(x, w, b)
    hard, soft = capi.softmax_xent(logits, ld), capi.softmax_xent_soft(logits, onehot)
    for a, c in zip(hard, soft):
        assert np.array_equal(u32(a), u32(c))
    if out == 3:
        mk = lambda *shape: T.full(shape, SENTINEL, device="cuda")
        hb, sb = [mk(B, 3), mk(B, 3), mk(B, 3), mk(B)], [mk(B, 3), mk(B, 3), mk(B, 3), mk(B)]
        capi.check(lib.cnn_linear_forward_softmax_xent(P(x), P(w), P(b), P(ld), *[P(t) for t in hb], B, n_in, 3, capi._stream()), "hard")
        capi.check(lib.cnn_linear_forward_softmax_xent_soft(P(x), P(w), P(b), P(onehot), *[P(t) for t in sb], B, n_in, 3, capi._stream()), "soft")
        for name, a, c in zip(NAMES, hb, sb):
            assert np.array_equal(u32(a), u32(c)), name


def _loss_from_terms(T, capi, terms_bits, B):
    terms = dev(T, terms_bits.view(np.float32))
    loss = T.zeros(1, device="cuda")
    capi.check(capi.load().cnn_loss_from_terms(capi._ptr(terms), capi._ptr(loss), B, capi._stream()), "cnn_loss_from_terms")
    return u32(loss)


worst_ratio = [0.0]


def _check_soft(T, x, w, b, ld, targets, relu, S, out):
    """one shape on real soft targets: logits / probs are the hard head's, delta = probs - targets in fp32, dx = linear_backward of that
    delta, the loss terms within (out + 4) * 2^-24 * sum |t log p| of float64 on the device's own probabilities (logf 2 ulp, a rounding
    per product and per addition), and the fused head equals cnn_linear_forward + cnn_softmax_xent_soft, the ordered loss sum included"""
    from cnn_amd import capi

    B = x.shape[0]
    ref = hard_head(T, x, w, b, ld, relu, S, out)
    got = soft_head(T, x, w, b, targets, relu, S, out)
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), "logits / probs"
    probs, th = got[1].view(np.float32), targets.cpu().numpy()
    delta = (probs - th).astype(np.float32)
    assert np.array_equal(got[2], delta.view(np.uint32)), "delta"
    _, _, dx = capi.linear_backward(x, dev(T, delta), w, float(B), relu_below=bool(relu))
    assert np.array_equal(got[4], u32(dx)), "dx"
    with np.errstate(divide="ignore"):
        prod = th.astype(np.float64) * np.log(probs.astype(np.float64))
    want, scale = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    err = np.abs(got[3].view(np.float32).astype(np.float64) - want)
    bound = (out + 4) * EPS32 * scale
    worst_ratio[0] = max(worst_ratio[0], float((err / bound).max()))
    assert np.all(err <= bound), (err / bound).max()
    logits = capi.linear_forward(x, w, b)
    gp, gd, gl = capi.softmax_xent_soft(logits, targets)
    assert np.array_equal(u32(logits), got[0]) and np.array_equal(u32(gp), got[1]) and np.array_equal(u32(gd), got[2]), "generic pair"
    assert np.array_equal(u32(gl), _loss_from_terms(T, capi, got[3], B)), "ordered loss sum"


@pytest.mark.parametrize("relu", [0, 1], ids=["plain", "relu_below"])
@pytest.mark.parametrize("S", SAMPLES)
def test_soft_head_on_soft_targets(T, S, relu):
    from cnn_amd import capi

    for n_in in WIDTHS:
        for B in BATCHES:
            x, w, b, ld, labels = case(T, B, n_in, relu)
            targets = capi.soft_targets(ld, 3, 0.1, 0.3, PAIR_FLIP, 0)
            _check_soft(T, x, w, b, ld, targets, relu, S, 3)
    print(f"worst loss-term error / bound so far: {worst_ratio[0]:.3f}")


@pytest.mark.parametrize("out", [8, 5])
def test_soft_head_generic_width(T, out):
    """out = 8 and 5: the S = 1 path whatever HEAD_SAMPLES says"""
    from cnn_amd import capi

    for relu in (0, 1):
        x, w, b, ld, labels = case(T, 5, 7000, relu, out)
        targets = capi.soft_targets(ld, out, 0.1, 0.3, PAIR_FLIP, 0)
        _check_soft(T, x, w, b, ld, targets, relu, 2, out)
    print(f"worst loss-term error / bound so far: {worst_ratio[0]:.3f}")
