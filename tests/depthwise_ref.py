"""The reference of the depthwise convolution (CNN_CONV2D_DEPTHWISE, architectures::DepthwiseConv2D), no device needed.

A depthwise convolution with filters w [C][1][k][k] IS the dense convolution with the block-diagonal filters expand_filters(w)
[C][C][k][k]: the off-diagonal zeros add exact zeros to every sum.  So the unchanged references hold it -- tests/exact.conv_truth on the
integer lattice (one correct bit pattern per element), the C oracle on continuous operands, oracle.pyoracle.SeqNet for a whole net
(expand_spec / expand_params / diag_grads) -- and the direct NumPy statement below (dw_f64 / dw_truth) is held to both by
tests/test_depthwise_reference.py.

A case is (B, C, H, W, k, s, pad); dense_case(case) is the (B, Ci, H, W, Co, k, s, pad) of tests/exact.py and tests/conv_route_cases.py."""
import numpy as np

from tests import exact as X

# ---- the cases of tests/test_gpu_depthwise.py (here, so that tests/test_depthwise_reference.py proves their conditions on the CPU) ----
K3_S1 = [(2, 5, 9, 9, 3, 1, 1), (1, 1, 3, 3, 3, 1, 1),
         (3, 37, 7, 7, 3, 1, 1),      # several planes per wave, a C tail
         (2, 40, 14, 14, 3, 1, 1), (2, 3, 30, 57, 3, 1, 0),
         (2, 2, 130, 67, 3, 1, 1),    # more rows and columns than one tile, tails both ways
         (1, 6, 5, 113, 3, 1, 1)]
K3_S2 = [(2, 5, 9, 9, 3, 2, 1),
         (2, 4, 10, 13, 3, 2, 0),     # even H: the last row is covered by no window and must come out +0
         (3, 33, 14, 14, 3, 2, 1), (2, 3, 56, 31, 3, 2, 1), (1, 2, 129, 66, 3, 2, 0)]
GENERIC = [(2, 3, 11, 12, 5, 1, 2), (2, 3, 13, 11, 5, 2, 0), (1, 2, 15, 9, 7, 2, 3), (2, 4, 6, 6, 1, 1, 0), (2, 3, 9, 9, 3, 3, 0)]
# Widths that are multiples of 4 and pads 0..4: with SHIFT_ROWS these reach every (kernel, stride, OFF / PP, vector flag) the 3x3 launches
# can choose (variants(), below; tests/test_depthwise_reference.py proves it) -- the lists above, all of odd widths, reach 9 of the 34.
VARIANT_S1 = [(2, 3, 8, 8, 3, 1, 1),
              (2, 40, 4, 4, 3, 1, 1),      # one strip, many planes per wave
              (2, 5, 20, 28, 3, 1, 1),     # three row tiles, seven strips
              (2, 3, 6, 12, 3, 1, 0),      # OFF 0
              (2, 3, 10, 10, 3, 1, 0),     # data gradient OFF 2 (Wo = 8); forward float4 stores behind scalar loads
              (2, 2, 7, 16, 3, 1, 2),      # OFF 2 forward
              (2, 3, 5, 6, 3, 1, 2),       # data gradient OFF 0 (Wo = 8)
              (1, 2, 5, 8, 3, 1, 3),       # OFF -1 by padding; the data gradient's pad' = -1
              (1, 2, 6, 12, 3, 1, 4)]      # pad' = -2
VARIANT_S2 = [(2, 3, 8, 8, 3, 2, 1), (2, 5, 20, 28, 3, 2, 1),
              (2, 3, 9, 12, 3, 2, 1),      # Wo = 6: float4 loads, scalar stores
              (2, 3, 9, 16, 3, 2, 0), (2, 3, 11, 9, 3, 2, 0), (2, 2, 7, 16, 3, 2, 2), (1, 2, 9, 8, 3, 2, 3), (2, 33, 4, 4, 3, 2, 1),
              (2, 3, 7, 11, 3, 2, 1)]
VARIANT_CASES = VARIANT_S1 + VARIANT_S2
ODD_WIDTH_CASES = K3_S1 + K3_S2 + GENERIC  # (run at SHIFTS_BOTH: everything aligned, and x / dy / w shifted by 4)
CASES = ODD_WIDTH_CASES + VARIANT_CASES
NARROW_CASES = [K3_S1[0], K3_S2[0]]  # one per stride on exact.NARROW
VARIANT_NARROW_CASES = [VARIANT_S1[2], VARIANT_S2[1]]
LARGEST = [K3_S1[5], K3_S2[4]]       # the planner-branch cases (by elements)

# byte shifts off the 256-byte boundary of (x and w, dy, the outputs, relu_below): each operand group alone, pairs, and 8 (off 16 bytes too)
SHIFT_ROWS = [(0, 0, 0, 0), (4, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4), (4, 0, 0, 0), (0, 4, 0, 0), (8, 8, 8, 8)]
SHIFTS_BOTH = [(0, 0, 0, 0), (4, 4, 0, 0)]
CALLS = ("forward", "forward_relu", "forward_relu/only", "backward_data", "backward_data_relu", "backward_weight")


def shifts_of(row):
    """a SHIFT_ROWS row -> the shift of every operand group of tests/depthwise_calls.Layer"""
    xw, dy, out, below = row
    return {"x": xw, "w": xw, "dy": dy, "out": out, "below": below}


def shift_key(row):
    return "shift" + "-".join(str(v) for v in row)


# ---- which code bodies a 3x3 launch chooses (conv_depthwise.hip: dw_off, vst, vdy), restated ----------------------------------------
def dw_off(aligned, IW, pad):
    """OFF of dw_load_row for rows of IW floats: -1 (scalar loads) unless the base is 16-byte aligned and IW % 4 == 0; then pad mod 4
    where that is at most 2"""
    if not aligned or IW % 4 != 0:
        return -1
    off = ((pad % 4) + 4) % 4
    return off if off <= 2 else -1


def launch_variants(case, shifts):
    """call (CALLS) -> (kernel, S, OFF or PP, v) of the specialised kernel the call launches: the kernel's family ("dw_fwd", "dw_dgrad",
    "dw_wgrad"), its stride, OFF of its row loads (PP = pad & 1 for the stride-2 data gradient) and whether it moves its outputs (the weight
    gradient: its dy) as float4.  Empty for a geometry of the generic kernels.  Every tensor starts on a 256-byte boundary plus its shift and
    planes are whole numbers of rows, so a tensor is 16-byte aligned iff its shift % 16 == 0."""
    B, C, H, W, k, s, pad, Ho, Wo = geometry(case)
    if k != 3 or s not in (1, 2):
        return {}
    al = {name: sh % 16 == 0 for name, sh in shifts.items()}
    fwd = ("dw_fwd", s, dw_off(al["x"], W, pad), int(Wo % 4 == 0 and al["out"]))
    out = {"forward": fwd, "forward_relu": fwd, "forward_relu/only": fwd}
    for call, below_ok in (("backward_data", True), ("backward_data_relu", al["below"])):
        v = int(W % 4 == 0 and al["out"] and below_ok)
        out[call] = ("dw_dgrad", s, dw_off(al["dy"], Wo, 2 - pad) if s == 1 else pad & 1, v)
    out["backward_weight"] = ("dw_wgrad", s, dw_off(al["x"], W, pad), int(Wo % 4 == 0 and al["dy"]))
    return out


def variants(case, shifts):
    """the set of (kernel, S, OFF or PP, v) the three passes of one case launch"""
    return set(launch_variants(case, shifts).values())


def tag_variant(kernel_key):
    """a kernel-timing key "dw_fwd<3x3,s2>|B2 ... p1 off1 v0" -> ("dw_fwd", 2, 1, 0); None for a key without the suffix"""
    import re

    m = re.fullmatch(r"(dw_\w+)<3x3,s([12])>\|.* (off|pp)(-?\d+) v([01])", kernel_key)
    if not m or (m.group(3) == "pp") != (m.group(1) == "dw_dgrad" and m.group(2) == "2"):  # (pp: the stride-2 data gradient, and only it)
        return None
    return (m.group(1), int(m.group(2)), int(m.group(4)), int(m.group(5)))


def key(case):
    return ",".join(str(v) for v in case)


def geometry(case):
    B, C, H, W, k, s, pad = case
    return B, C, H, W, k, s, pad, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def dense_case(case):
    B, C, H, W, k, s, pad = case
    return (B, C, H, W, C, k, s, pad)


def headroom(case, amp=8, bias_amp=64):
    """the largest possible sum |term| over the three passes: forward k*k products + the bias, data gradient k*k products, weight
    gradient B * Ho * Wo products (tests/exact.headroom with one input channel per output)"""
    B, C, H, W, k, s, pad, Ho, Wo = geometry(case)
    return max(amp * amp * k * k + bias_amp, amp * amp * k * k, amp * amp * B * Ho * Wo)


# ---- depthwise <-> block-diagonal dense -------------------------------------------------------------------------------------------
def expand_filters(w):
    """[C][1][k][k] -> block-diagonal [C][C][k][k]"""
    w = np.asarray(w)
    C, one, k, _ = w.shape
    assert one == 1
    out = np.zeros((C, C, k, k), w.dtype)
    idx = np.arange(C)
    out[idx, idx] = w[:, 0]
    return out


def diag_filters(W):
    """the diagonal of [C][C][k][k] as [C][1][k][k]"""
    W = np.asarray(W)
    idx = np.arange(W.shape[0])
    return np.ascontiguousarray(W[idx, idx][:, None])


def expand_spec(spec, in_channels=3):
    """a cnn_amd.stacks spec with every ("dwconv", k, s, pad) replaced by the dense ("conv", C, k, s, pad) on its C input channels"""
    out, C = [], in_channels
    for item in spec:
        if item[0] == "dwconv":
            out.append(("conv", C, item[1], item[2], item[3]))
        else:
            out.append(item)
            if item[0] == "conv":
                C = item[1]
            elif item[0] == "linear":
                C = item[1]
    return out


def _blocks(layout):
    """(entry, offset in the depthwise net's flat vector, offset in the expanded net's) per layer"""
    off, xoff = 0, 0
    for e in layout:
        yield e, off, xoff
        off += e["params"]
        if e["kind"] == "dwconv":
            C, k = e["in"][0], e["k"]
            xoff += C * C * k * k + C
        else:
            xoff += e["params"]


def expanded_count(layout):
    return sum((e["in"][0] ** 2 * e["k"] ** 2 + e["in"][0]) if e["kind"] == "dwconv" else e["params"] for e in layout)


def expand_params(layout, flat):
    """flat parameters (or any vector in checkpoint order) of a net with dwconv layers (layout = cnn_amd.stacks.walk of its spec) -> the
    flat vector of the expand_spec net: block-diagonal filters, everything else verbatim"""
    flat = np.asarray(flat)
    out = np.zeros(expanded_count(layout), flat.dtype)
    for e, off, xoff in _blocks(layout):
        n = e["params"]
        if e["kind"] == "dwconv":
            C, k = e["in"][0], e["k"]
            nw = C * k * k
            out[xoff:xoff + C * C * k * k] = expand_filters(flat[off:off + nw].reshape(C, 1, k, k)).ravel()
            out[xoff + C * C * k * k:xoff + C * C * k * k + C] = flat[off + nw:off + n]
        else:
            out[xoff:xoff + n] = flat[off:off + n]
    return out


def diag_grads(layout, flat_expanded):
    """the inverse on a gradient (or parameter) vector of the expanded net: the diagonal blocks of every expanded dwconv layer"""
    flat_expanded = np.asarray(flat_expanded)
    out = np.zeros(sum(e["params"] for e in layout), flat_expanded.dtype)
    for e, off, xoff in _blocks(layout):
        n = e["params"]
        if e["kind"] == "dwconv":
            C, k = e["in"][0], e["k"]
            nw = C * k * k
            out[off:off + nw] = diag_filters(flat_expanded[xoff:xoff + C * C * k * k].reshape(C, C, k, k)).ravel()
            out[off + nw:off + n] = flat_expanded[xoff + C * C * k * k:xoff + C * C * k * k + C]
        else:
            out[off:off + n] = flat_expanded[xoff:xoff + n]
    return out


# ---- the three passes, stated directly ----------------------------------------------------------------------------------------------
def dw_f64(case, x, w, b, dy):
    """y, the undivided S_gw [C][1][k][k] and S_gb [C], dx -- all float64.  y[b][c] = bias[c] + x[b][c] (*) w[c] over the zero-padded
    input; S_gw[c] = sum_b sum_pq dy * x; S_gb[c] = sum dy; dx = the scatter of dy * w over the taps, cropped back (rows and columns no
    window covers stay 0)"""
    B, C, H, W, k, s, pad, Ho, Wo = geometry(case)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64).reshape(C, k, k), dy.astype(np.float64)
    xp = np.pad(x64, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(2, 3))[:, :, ::s, ::s]  # [B][C][Ho][Wo][k][k]
    assert win.shape == (B, C, Ho, Wo, k, k), win.shape
    y = np.einsum("bcpqij,cij->bcpq", win, w64) + b.astype(np.float64)[None, :, None, None]
    S_gw = np.einsum("bcpq,bcpqij->cij", dy64, win).reshape(C, 1, k, k)
    S_gb = dy64.sum(axis=(0, 2, 3))
    dxp = np.zeros_like(xp)
    for i in range(k):
        for j in range(k):
            dxp[:, :, i:i + s * Ho:s, j:j + s * Wo:s] += dy64 * w64[None, :, i, j, None, None]
    dx = dxp[:, :, pad:pad + H, pad:pad + W]
    return np.ascontiguousarray(y), S_gw, S_gb, np.ascontiguousarray(dx)


def dw_truth(case, x, w, b, dy):
    """dw_f64 on lattice operands as the one correct fp32 pattern: y and dx float32 (checked exact), the sums undivided in float64"""
    y, S_gw, S_gb, dx = dw_f64(case, x, w, b, dy)
    assert max(np.abs(S_gw).max(), np.abs(S_gb).max()) < X.LIMIT
    return X._f32(y), S_gw, S_gb, X._f32(dx)


def lattice_inputs(case, seed, amp=8, bias_amp=64):
    """x, w [C][1][k][k], b, dy: float32 integers in [-amp, amp] (bias: [-bias_amp, bias_amp])"""
    B, C, H, W, k, s, pad, Ho, Wo = geometry(case)
    assert headroom(case, amp, bias_amp) < X.LIMIT, (case, amp, bias_amp)
    rs = np.random.RandomState(seed)
    return X._ints(rs, amp, (B, C, H, W)), X._ints(rs, amp, (C, 1, k, k)), X._ints(rs, bias_amp, (C,)), X._ints(rs, amp, (B, C, Ho, Wo))


_MEMO = {}


def lattice_case(case, lattice=X.WIDE):
    """(x, w, b, dy, relu_below), (y, S_gw, S_gb, dx) of one case on one lattice, computed once and handed out read-only; relu_below =
    max(x, 0): a ReLU layer's output on the integer x, zero at about half of the positions"""
    k_ = ("lattice", tuple(case), tuple(lattice))
    if k_ not in _MEMO:
        x, w, b, dy = lattice_inputs(case, 7100 + lattice[0], *lattice)
        ins = (x, w, b, dy, np.maximum(x, np.float32(0)))
        truth = dw_truth(case, x, w, b, dy)
        for a in ins + truth:
            a.flags.writeable = False
        _MEMO[k_] = (ins, truth)
    return _MEMO[k_]


def continuous_case(case):
    """(x, w, b, dy, relu_below) from tests/util's seeded generators, and the C oracle's (y, gw / B-averaged, gb, dx) on the expanded
    filters with the diagonal taken back out; once per case, read-only"""
    from oracle import pyoracle as O
    from tests import util

    k_ = ("continuous", tuple(case))
    if k_ not in _MEMO:
        B, C, H, W, k, s, pad, Ho, Wo = geometry(case)
        seed = 9100 + sum(case)
        x = util.uniform_pm1(seed, (B, C, H, W))
        w = util.normal_scaled(seed + 1, (C, 1, k, k))
        b = util.normal_scaled(seed + 2, (C,))
        dy = util.uniform_pm1(seed + 3, (B, C, Ho, Wo))
        below = np.maximum(util.uniform_pm1(seed + 4, (B, C, H, W)), np.float32(0))
        Wd = expand_filters(w)
        y = O.conv2d_forward_padded(x, Wd, b, s, pad)
        gw, gb, dx = O.conv2d_backward_padded(x, dy, Wd, s, pad)
        ins, ref = (x, w, b, dy, below), (y, diag_filters(gw), gb, dx)
        for a in ins + ref:
            a.flags.writeable = False
        _MEMO[k_] = (ins, ref)
    return _MEMO[k_]
