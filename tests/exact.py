"""Operands on an integer lattice, and the one correct bit pattern of every convolution / linear output on them (no device needed).

The tolerance checks (tests/util.assert_close) allow 1e-4 of a tensor's maximum because fp32 sums in another order round differently.
With x, w, dy in {-amp..amp} and the bias in {-bias_amp..bias_amp} nothing rounds at all: every product is an integer, and every partial
sum of ANY subset of an output's terms is an integer of magnitude <= headroom() < 2^24, which fp32 holds exactly -- in any order and
grouping, with or without FMA, on the VALU or the matrix pipe, in one slab or in fifty.  So there is one correct fp32 value per element,
every route of the library must produce it, and a difference is never rounding: it is a term that is missing, doubled or misplaced (it
reads as an integer in bits_equal's report), a decision at 0 or at a tie that differs from the reference's, or a division that is not
the correctly rounded sum / divisor that include/cnn_amd.h promises.  Exact zeros and exact ties, which continuous operands never give,
are common here (most of all on the narrow lattice amp=1, bias_amp=2).

conv_truth / linear_truth state the operations directly in NumPy, in float64 through BLAS (exact below 2^53).  tests/test_exact_reference.py
holds them to the fp32 C oracle bit for bit on the CPU, which is the evidence that the lattice claim holds under the reference's own
summation order."""
import numpy as np

NARROW = (1, 2)   # (amp, bias_amp): x, w in {-1, 0, 1}, bias in {-2..2} -- few distinct values: the most zeros and ties
WIDE = (8, 64)    # the default lattice
LIMIT = 2 ** 24   # every integer of magnitude <= 2^24 is an fp32 value


# ---- the cases of tests/test_gpu_exact_sums.py (here, so that tests/test_exact_reference.py proves its conditions without a device) -----
# the first block in the pooled domain: (B, H, W) of (B, 3, H, W, 16, 3, 2, 0), narrow lattice
FIRST_BLOCK_SHAPES = [(2, 56, 56), (3, 37, 41), (2, 12, 20), (5, 7, 5), (2, 30, 26)]
# 1x1 layers whose weight gradient takes the c11_wgrad_kernel<3>, <5>, <6> and <7> instances (conv_1x1.hip), which no other test launches
C11_CASES = [(2, 48, 7, 9, 32, 1, 1, 0), (2, 80, 7, 9, 48, 1, 2, 0), (2, 96, 6, 6, 32, 1, 1, 0), (2, 112, 5, 8, 144, 1, 2, 0)]
LINEAR_SHAPES = [(4, 4608, 3), (3, 100, 10), (5, 33, 17), (37, 130, 8), (256, 4608, 3), (1, 7, 1), (19, 25088, 3), (33, 6000, 2)]
# the seed of a desc's lattice operands; the listed ones were chosen so that the truth holds at least one y == 0 (tests/test_exact_reference.py
# asserts it for every desc): these layers have a few hundred outputs each and most seeds give none
_SEEDS = {((2, 3, 9, 9, 16, 3, 2, 0), 8): 7010, ((2, 3, 9, 5, 7, 3, 1, 0), 8): 7010, ((2, 5, 13, 11, 7, 5, 2, 0), 8): 7011}


def seed_of(case, amp=8):
    return _SEEDS.get((tuple(case[:8]), amp), 7000 + amp)


def geometry(case):
    B, Ci, H, W, Co, k, s, pad = case[:8]
    return B, Ci, H, W, Co, k, s, pad, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def headroom(case, amp=8, bias_amp=64, dy_amp=None, dy_terms=None):
    """the largest possible sum |term| over the three passes of one desc: forward amp^2 * Ci * k * k + bias_amp, data gradient
    amp^2 * Co * k * k, weight gradient amp^2 * B * Ho * Wo.  This bound is the whole argument for exactness: every term is an integer,
    so every partial sum of any subset of the terms of an output element, taken in any order, is an integer of magnitude <= headroom,
    and below 2^24 every such integer is an fp32 value -- no addition, fused or not, ever rounds.
    dy_amp: |dy| <= dy_amp instead of amp (the pooled-domain gradients, whose dy is a routed dpool); dy_terms: at most that many non-zero
    dy per channel instead of B * Ho * Wo (one per pooling window)."""
    B, Ci, H, W, Co, k, s, pad, Ho, Wo = geometry(case)
    dy_amp = amp if dy_amp is None else dy_amp
    terms = B * Ho * Wo if dy_terms is None else dy_terms
    return max(amp * amp * Ci * k * k + bias_amp, dy_amp * amp * Co * k * k, dy_amp * amp * terms)


def linear_headroom(B, n_in, n_out, amp=8, bias_amp=64):
    """forward amp^2 * n_in + bias_amp, data gradient amp^2 * n_out, weight gradient amp^2 * B (see headroom)"""
    return max(amp * amp * n_in + bias_amp, amp * amp * n_out, amp * amp * B)


def _ints(rs, amp, shape):
    return rs.randint(-amp, amp + 1, size=shape).astype(np.float32)


def lattice_inputs(case, seed, amp=8, bias_amp=64):
    """x, w, b, dy of one desc: float32 arrays of integers in [-amp, amp] (bias: [-bias_amp, bias_amp]) from RandomState(seed).randint"""
    B, Ci, H, W, Co, k, s, pad, Ho, Wo = geometry(case)
    assert headroom(case, amp, bias_amp) < LIMIT, (case, amp, bias_amp, headroom(case, amp, bias_amp))
    rs = np.random.RandomState(seed)
    return _ints(rs, amp, (B, Ci, H, W)), _ints(rs, amp, (Co, Ci, k, k)), _ints(rs, bias_amp, (Co,)), _ints(rs, amp, (B, Co, Ho, Wo))


def linear_inputs(B, n_in, n_out, seed, amp=8, bias_amp=64):
    """x, w, b, dy of one linear layer on the lattice"""
    assert linear_headroom(B, n_in, n_out, amp, bias_amp) < LIMIT
    rs = np.random.RandomState(seed)
    return _ints(rs, amp, (B, n_in)), _ints(rs, amp, (n_in, n_out)), _ints(rs, bias_amp, (n_out,)), _ints(rs, amp, (B, n_out))


def _f32(a):
    """float64 integers -> float32, checked to be exact; + 0.0: a sum of products is never -0 once +0 or a bias has been added"""
    out = (a + 0.0).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), a), "truth outside the fp32 integers: headroom was not checked"
    return out


_TRUTH_MEMO = {}


def conv_truth(case, x, w, b, dy, memo=None):
    """y, S_gw, S_gb, dx of the padded convolution: y and dx as float32, S_gw = sum_{b,p,q} dy * x and S_gb = sum dy UNDIVIDED in
    float64 (see divided).  Forward and weight gradient over the sliding windows of the zero-padded input, the data gradient as the
    scatter of dy * w over the taps, cropped back: rows and columns behind the last window stay 0.
    memo: a hashable key (case, seed, amp, ...) the inputs were made from, unchanged -- computed once per key and handed out read-only
    (the way tests/test_gpu_parity._oracle_conv does)"""
    if memo is not None and memo in _TRUTH_MEMO:
        return _TRUTH_MEMO[memo]
    y, S_gw, S_gb, dx = conv_f64(case, x, w, b, dy)
    assert max(np.abs(S_gw).max(), np.abs(S_gb).max()) < LIMIT
    out = (_f32(y), S_gw, S_gb, _f32(dx))
    if memo is not None:
        for a in out:
            a.flags.writeable = False
        _TRUTH_MEMO[memo] = out
    return out


def conv_f64(case, x, w, b, dy):
    """the arithmetic of conv_truth in float64 on any operands: y, the undivided S_gw and S_gb, dx (all float64).  On continuous operands
    it is a high-precision reference of the same operation, for any filter size -- the C oracle transcribes the reference's walk over
    window centres (r = (k - 1) / 2 on either side) and is the operation only for odd k"""
    B, Ci, H, W, Co, k, s, pad, Ho, Wo = geometry(case)
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(2, 3))[:, :, ::s, ::s]          # [B][Ci][Ho][Wo][k][k]
    assert win.shape == (B, Ci, Ho, Wo, k, k), win.shape
    cols = np.ascontiguousarray(win.transpose(0, 2, 3, 1, 4, 5)).reshape(B * Ho * Wo, Ci * k * k)    # rows (b,p,q), columns (ci,i,j)
    wm = w.astype(np.float64).reshape(Co, Ci * k * k)
    dym = np.ascontiguousarray(dy.astype(np.float64).transpose(0, 2, 3, 1)).reshape(B * Ho * Wo, Co)
    y = (cols @ wm.T + b.astype(np.float64)).reshape(B, Ho, Wo, Co).transpose(0, 3, 1, 2)
    S_gw = (dym.T @ cols).reshape(Co, Ci, k, k)
    S_gb = dym.sum(axis=0)
    dcols = (dym @ wm).reshape(B, Ho, Wo, Ci, k, k)
    dxp = np.zeros_like(xp)
    for i in range(k):
        for j in range(k):
            dxp[:, :, i : i + s * Ho : s, j : j + s * Wo : s] += dcols[..., i, j].transpose(0, 3, 1, 2)
    dx = dxp[:, :, pad : pad + H, pad : pad + W]
    return np.ascontiguousarray(y), S_gw, S_gb, np.ascontiguousarray(dx)


def lattice_conv(case, seed, amp=8, bias_amp=64):
    """(x, w, b, dy), (y, S_gw, S_gb, dx): lattice_inputs and their conv_truth, once per (case, seed, amp, bias_amp)"""
    key = ("conv", tuple(case[:8]), seed, amp, bias_amp)
    if key not in _TRUTH_MEMO:
        ins = lattice_inputs(case, seed, amp, bias_amp)
        for a in ins:
            a.flags.writeable = False
        _TRUTH_MEMO[key] = (ins, conv_truth(case, *ins))
    return _TRUTH_MEMO[key]


def linear_truth(x, w, b, dy):
    """y, S_gW, S_gb, dx of y = x W + b with W [n_in][n_out]: y and dx float32, the sums over the batch undivided in float64"""
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    return _f32(x64 @ w64 + b.astype(np.float64)), x64.T @ dy64, dy64.sum(axis=0), _f32(dy64 @ w64.T)


def divided(S, divisor):
    """the correctly rounded quotient of the exact sum: what "gw = (sum) / divisor" (include/cnn_amd.h) promises.  Not the oracle's
    per-sample division, which agrees with it only where the divisor is a power of two."""
    S32 = np.asarray(S).astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S)
    return (S32 / np.float32(divisor)).astype(np.float32)


# ---- the first block in the pooled domain: conv -> ReLU -> MaxPool2D(2, 2) --------------------------------------------------------
def first_block_truth(case, seed, amp=1, bias_amp=2, dpool_amp=8):
    """{x, w, b, y, relu, pooled, mask, dead, dpool, dy, S_gw, S_gb, dx} of one (B, 3, H, W, 16, 3, 2, 0) desc.  relu = max(y, 0) on the
    exact y; pooled and mask are the ORACLE's maxpool_forward of it -- its tie rule is the contract, it is not restated here; dead =
    pooled <= 0 (bit 31 of the int32 mask, bit 7 of the packed one).  dpool: integers in {-dpool_amp..dpool_amp}; dy = the oracle's
    relu_backward(relu, maxpool_backward(dpool, mask)): at most one non-zero per window; S_gw, S_gb, dx = conv_truth with that dy."""
    from oracle import pyoracle as O

    key = ("first_block", tuple(case[:8]), seed, amp, bias_amp, dpool_amp)
    if key in _TRUTH_MEMO:
        return _TRUTH_MEMO[key]
    B, Ci, H, W, Co, k, s, pad, Ho, Wo = geometry(case)
    PHo, PWo = Ho // 2, Wo // 2
    assert headroom(case, amp, bias_amp, dy_amp=dpool_amp, dy_terms=B * PHo * PWo) < LIMIT
    x, w, b, dy0 = lattice_inputs(case, seed, amp, bias_amp)
    y = conv_truth(case, x, w, b, dy0)[0]
    relu = np.maximum(y, np.float32(0))
    pooled, mask = O.maxpool_forward(relu, 2, 2)
    dpool = _ints(np.random.RandomState(seed + 1), dpool_amp, pooled.shape)
    dy = O.relu_backward(relu, O.maxpool_backward(dpool, mask, relu.shape, 2, 2))
    assert np.count_nonzero(dy) <= B * Co * PHo * PWo
    _, S_gw, S_gb, dx = conv_truth(case, x, w, b, dy)
    t = dict(x=x, w=w, b=b, y=y, relu=relu, pooled=pooled, mask=mask, dead=pooled <= 0, dpool=dpool, dy=dy, S_gw=S_gw, S_gb=S_gb, dx=dx)
    for a in t.values():
        a.flags.writeable = False
    _TRUTH_MEMO[key] = t
    return t


def window_shares(relu):
    """(windows, all-zero windows, windows whose positive maximum sits at two or more of the four window positions) of the 2x2 / step-2
    pooling of relu -- conditions on the inputs, from the truth alone"""
    B, C, Ho, Wo = relu.shape
    PHo, PWo = Ho // 2, Wo // 2
    win = relu[:, :, : 2 * PHo, : 2 * PWo].reshape(B, C, PHo, 2, PWo, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, PHo, PWo, 4)
    top = win.max(axis=-1)
    tied = (top > 0) & ((win == top[..., None]).sum(axis=-1) >= 2)
    return top.size, int((top <= 0).sum()), int(tied.sum())


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def bits_differ(a, truth, what, unit=1.0):
    """None when a and truth hold the same fp32 bit patterns, else the report: how many elements differ, the first index, both values
    and their difference in lattice units (unit = 1 for sums, 1 / divisor for divided ones): a missing or doubled term reads as an
    integer, a wrong division as a fraction of one"""
    a, truth = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(truth, np.float32)
    if a.shape != truth.shape:
        return f"{what}: shape {a.shape}, truth {truth.shape}"
    bad = a.view(np.uint32) != truth.view(np.uint32)
    if not bad.any():
        return None
    first = tuple(int(i) for i in np.argwhere(bad)[0])
    d = (np.float64(a[first]) - np.float64(truth[first])) / unit
    return (f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at {first}: got {a[first]!r} ({a.view(np.uint32)[first]:#010x}), "
            f"truth {truth[first]!r} ({truth.view(np.uint32)[first]:#010x}), difference {d:+.6g} lattice units")


def bits_equal(a, truth, what, unit=1.0):
    report = bits_differ(a, truth, what, unit)
    assert report is None, report
