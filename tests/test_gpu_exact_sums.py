"""Every convolution and linear route on lattice operands, bit for bit against the integer truth (tests/exact.py).

x, w, dy are integers in {-8..8} and the bias in {-64..64} (the narrow lattice: {-1, 0, 1} and {-2..2}), so every partial sum of every
output, in any order and grouping, is an fp32 integer: there is ONE correct bit pattern per element, and every kernel family, option, CU
count, slab split, prepared or plain call, with the workspace given, withheld or misaligned, must produce it.  Exact zeros and exact ties
are common, so the decisions `v >= 0 ? v : 0`, `relu_below <= 0` and the first-maximum rule of the fused first block see them.  The
weight gradients are held to the correctly rounded (sum) / divisor of include/cnn_amd.h, for divisors 1 and 4 everywhere and 3 on one
desc per family.  tests/test_exact_reference.py proves the instrument on the CPU.

The calls are the ones tests/conv_route_cases.py walks for tests/golden/conv_routes.json; at default options each call's launch log must
equal the golden one of the same desc (routes depend on the desc, not on the data), so no family is silently skipped.

Not held to this: anything through expf, logf, sqrt or a per-sample division (softmax, the loss, BatchNorm, the optimizers)."""
import collections
import json
import os
import re

import numpy as np
import pytest

from tests import conv_route_cases as R
from tests import exact as X

pytestmark = pytest.mark.gpu

HP = R.HAND_PICKED
FIRST_LAYER = [HP[0], HP[1], HP[2]]
NARROW_CASES = FIRST_LAYER + [HP[11], HP[14]]  # ... and two mid-size descs: (2,64,13,13,128,3,2,0) and (2,32,28,28,128,3,1,1)
# one desc per weight-gradient family, by the kernel the golden launch log names for it
DIV3_CASES = {"conv_wgrad_win<": HP[1], "wgrad_rd<": HP[24], "conv_wgrad_os<": HP[11], "wgrad_sp<": HP[13], "wgrad_sp2<": HP[25],
              "wgrad_sp_any<": HP[21], "conv_stem_wgrad<": HP[3], "conv_1x1/wgrad": HP[5], "wgrad_kernel<": HP[26]}
# the switches that move a desc to another family (or another body of the same one), and the descs each is run over
SWITCH_RUNS = ([(n, v, c) for n, v in R.OPTIONS for c in R.OPTION_CASES]
               + [("CONV_ROWS", "0", c) for c in R.ROWS_CASES]
               + [("ROWS_ANY", "0", c) for c in (HP[17], HP[18], HP[19])]
               + [("WGRAD_SP_ANY", v, c) for v in ("0", "2") for c in (HP[21], HP[22], HP[13], HP[14])]
               + [("CONV_1X1", "0", c) for c in (HP[5], HP[6])])
_id = lambda c: R.key(c)
_lat = lambda l: "amp%d" % l[0]

HELD = collections.Counter()  # kernel (launch-log name without its template arguments) -> (desc, call, option) triples held to exact bits


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    arch = capi.load().cnn_amd_device_arch().decode()
    assert arch == "gfx950", f"built for gfx950, running on {arch}"
    yield torch
    print("\n(desc, call, option) triples held to exact bits, by kernel:")
    for name, n in sorted(HELD.items()):
        print(f"  {name}: {n}")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "conv_routes.json")))


def dev(T, a):
    return T.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the truths and their inputs are handed out read-only)


def host(t):
    return t.detach().cpu().numpy()


def _layer(T, case, lattice, divisor):
    (x, w, b, dy), truth = X.lattice_conv(case, X.seed_of(case, lattice[0]), *lattice)
    relu_below = np.maximum(x, np.float32(0))  # a ReLU layer's output on the integer x: zero at about half of the positions
    return R._Layer(T, case, 0, inputs=tuple(np.array(a) for a in (x, w, b, dy, relu_below)), divisor=divisor), truth, relu_below


def _want(call, out, truth, relu_below, divisor):
    """the one correct tensor of output `out` of call `call`, and its lattice unit"""
    y, S_gw, S_gb, dx = truth
    if out == "y":
        return y, 1.0
    if out == "y_relu":
        return np.maximum(y, np.float32(0)), 1.0
    if out == "dx":
        return (np.where(relu_below <= 0, np.float32(0), dx) if "backward_data_relu" in call else dx), 1.0
    return X.divided({"gw": S_gw, "gb": S_gb}[out], divisor), 1.0 / divisor


def _hold(T, L, calls, truth, relu_below, golden_calls, option, check_log=True):
    """runs every call with the launch log on and holds each output to the truth; golden_calls: the golden record of this desc (None: a
    desc it does not hold) -- a call may refuse only where the record refuses, with the same code; with check_log (default options) a
    call recorded as refused must refuse and the launch log must be the recorded one; without it (under a switch) the calls that withhold
    or misalign the workspace may also refuse with CNN_AMD_E_BADARG.  All differences of one desc are reported together."""
    wrong = []
    for name, fn in calls.items():
        out, log = R._logged_outputs(T, fn)
        rec = golden_calls[name] if golden_calls is not None else None
        if isinstance(out, int):
            if not check_log and "/" in name and out == 1:
                continue  # (under a switch, the family that takes over may need the workspace this call withholds or misaligns)
            if rec is None or rec.get("rc") != out:
                wrong.append(f"{name}: refused with code {out}, recorded: {rec.get('rc', 'success') if rec else 'nothing'}")
            continue
        if rec is not None and "rc" in rec and check_log:
            wrong.append(f"{name}: recorded as refused with code {rec['rc']}, succeeded")
            continue
        if rec is not None and check_log and log != rec["log"]:
            wrong.append(f"{name}: launch log {log}, recorded {rec['log']}")
        bad = False
        for o, t in sorted(out.items()):
            want, unit = _want(name, o, truth, relu_below, L.divisor)
            report = X.bits_differ(host(t), want, f"{name}: {o}", unit)
            if report:
                wrong.append(report)
                bad = True
        if not bad:
            for k in log:
                HELD[re.sub(r"<[^>]*>", "", k.split("|")[0])] += 1
    assert not wrong, f"{R.key(L.case)} [{option}], divisor {L.divisor}:\n" + "\n".join(wrong)


def _all_calls(T, L):
    """the unprepared calls of conv_route_cases, then one prepare_filters and the prepared ones"""
    calls = dict(R._calls(L, L.case in R.ROWS_CASES))
    from cnn_amd import capi

    pf, pd = L.conv.prepared_buffers()
    pf.fill_(0x5A), pd.fill_(0x5A)
    capi.prepare_filters([L.conv], [L.w], [L.b], [pf], [pd])
    calls.update(R._prepared_calls(L, pf, pd))
    return calls


def _cases_lattices():
    return [(c, X.WIDE) for c in HP] + [(c, X.NARROW) for c in NARROW_CASES]


@pytest.mark.parametrize("case,lattice", _cases_lattices(), ids=lambda v: _id(v) if len(v) > 2 else _lat(v))
def test_every_call_of_every_desc_is_exact(T, golden, case, lattice):
    """forward, forward + ReLU, both data gradients, the weight gradient (divisor 1), the calls without a workspace and with a misaligned
    one, and the prepared calls, at default options: exact bits and the golden launch log"""
    L, truth, relu_below = _layer(T, case, lattice, 1.0)
    _hold(T, L, _all_calls(T, L), truth, relu_below, golden[R.key(case)], "default")


def _divisor_runs():
    runs = [(c, l, 4.0) for c, l in _cases_lattices()]
    return runs + [(c, X.WIDE, 3.0) for c in DIV3_CASES.values()]


@pytest.mark.parametrize("case,lattice,divisor", _divisor_runs(), ids=lambda v: _id(v) if isinstance(v, tuple) and len(v) > 2 else (_lat(v) if isinstance(v, tuple) else "div%g" % v))
def test_weight_gradient_is_the_rounded_quotient_of_the_exact_sum(T, golden, case, lattice, divisor):
    """gw = (sum) / divisor, gb likewise: divisor 4 (exact) on every desc, 3 on one desc per family -- the correctly rounded quotient of
    the exact sum, which sum * (1 / 3) or a division per slab does not give"""
    L, truth, relu_below = _layer(T, case, lattice, divisor)
    calls = {"backward_weight": R._calls(L, False)["backward_weight"]}
    _hold(T, L, calls, truth, relu_below, golden[R.key(case)], "default")


def test_divisor_three_descs_cover_the_families(golden):
    for prefix, case in DIV3_CASES.items():
        assert any(k.startswith(prefix) for k in golden[R.key(case)]["backward_weight"]["log"]), (prefix, case)


def _switched(T, golden, lib_option, name, value, case, lattice=X.WIDE):
    """all calls under one switch (the launch log is taken and not asserted: what a switch moves is documented per switch), then at the
    default again, where the golden log holds"""
    lib_option(name, value)
    L, truth, relu_below = _layer(T, case, lattice, 4.0)  # (built under the switch: plans, workspaces and prepared images belong to it)
    _hold(T, L, _all_calls(T, L), truth, relu_below, golden.get(R.key(case)), f"{name}={value}", check_log=False)
    lib_option(name, None)
    L, truth, relu_below = _layer(T, case, lattice, 4.0)
    _hold(T, L, _all_calls(T, L), truth, relu_below, golden.get(R.key(case)), f"default after {name}={value}")


@pytest.mark.parametrize("name,value,case", SWITCH_RUNS, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_every_call_is_exact_under_a_switch(T, golden, lib_option, name, value, case):
    _switched(T, golden, lib_option, name, value, case)


def _cu_cases():
    from tests.test_gpu_cu_counts import DETERMINISM_CASES

    return DETERMINISM_CASES


@pytest.mark.parametrize("cus", ["1", "5"])
@pytest.mark.parametrize("case", _cu_cases(), ids=_id)
def test_every_call_is_exact_at_another_cu_count(T, golden, lib_option, case, cus):
    """one desc per family with the planners told the card has 1 and 5 compute units: other slab counts, other shares per workgroup --
    the order of every sum moves, its bits must not"""
    _switched(T, golden, lib_option, "CUS", cus, case)


def _im2col_cases():
    from tests.test_gpu_parity import CONV_CASES

    return CONV_CASES[:5] + CONV_CASES[9:]


@pytest.mark.parametrize("divisor", [1.0, 3.0, 4.0], ids=lambda d: "div%g" % d)
@pytest.mark.parametrize("case", _im2col_cases(), ids=_id)
def test_im2col_entries_are_exact(T, case, divisor):
    """cnn_conv2d_forward_im2col / backward_weight_im2col / backward_data_im2col on the descs of test_conv2d_im2col_fallback_vs_oracle"""
    from cnn_amd import capi

    (x, w, b, dy), (y, S_gw, S_gb, dx) = X.lattice_conv(case, X.seed_of(case), *X.WIDE)
    conv = capi.Conv2d(*case)
    xd, wd, bd, dyd = dev(T, x), dev(T, w), dev(T, b), dev(T, dy)
    if divisor == 1.0:
        X.bits_equal(host(conv.forward_im2col(xd, wd, bd)), y, "im2col y")
        X.bits_equal(host(conv.backward_data_im2col(dyd, wd)), dx, "im2col dx")
    gw, gb = conv.backward_weight_im2col(xd, dyd, divisor)
    X.bits_equal(host(gw), X.divided(S_gw, divisor), "im2col gw", 1.0 / divisor)
    X.bits_equal(host(gb), X.divided(S_gb, divisor), "im2col gb", 1.0 / divisor)
    HELD["im2col entries"] += 1


# ---- the first block in the pooled domain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [0, 1], ids=["window_per_lane", "lane_pair"])
@pytest.mark.parametrize("packed", [False, True], ids=["int32_mask", "packed_mask"])
@pytest.mark.parametrize("shape", X.FIRST_BLOCK_SHAPES, ids=lambda s: "B%d_%dx%d" % s)
def test_first_block_in_the_pooled_domain_is_exact(T, lib_option, shape, packed, pair):
    """conv -> ReLU -> MaxPool2D(2, 2) fused, on the narrow lattice: 10-17 % of the windows are all zero and 8-16 % have their positive
    maximum at two or more positions (asserted in tests/test_exact_reference.py).  Pooled values = the oracle's pool of the exact
    relu(y); the argmax part of the mask = the oracle's first-maximum rule; the mark (bit 31, bit 7 of the packed byte) = pooled <= 0;
    the gradients from an integer dpool = the truth with dy = the oracle's ReLU and pool backward of it.  Plain and prepared filters,
    both forward bodies (FWD_POOL_PAIR), both mask forms."""
    from cnn_amd import capi

    if pair:
        lib_option("FWD_POOL_PAIR", "1")
    B, H, W = shape
    case = (B, 3, H, W, 16, 3, 2, 0)
    t = X.first_block_truth(case, X.seed_of(case, 1))
    conv = capi.Conv2d(*case)
    assert conv.relu_maxpool2_supported()
    if packed:
        assert conv.pool_mask_packed_supported()
        conv.set_pool_mask_packed()
    xd, wd, bd, dpool = dev(T, t["x"]), dev(T, t["w"]), dev(T, t["b"]), dev(T, t["dpool"])
    PHo, PWo = t["pooled"].shape[2:]
    pf, pd = conv.prepared_buffers("cuda")
    capi.prepare_filters([conv], [wd], [bd], [pf], [pd])
    want_mask = (t["mask"].astype(np.int64) | (t["dead"].astype(np.int64) << 31)).astype(np.uint32).view(np.int32)

    def new_mask():
        if packed:
            return T.full((conv.pool_mask_bytes(),), 0x55, dtype=T.uint8, device="cuda")
        return T.full((B, 16, PHo, PWo), -1, dtype=T.int32, device="cuda")

    def as_int32(mask):
        if not packed:
            return host(mask)
        pitch = (PWo + 3) & ~3
        rows = host(mask)[: B * 16 * PHo * pitch].reshape(B, 16, PHo, pitch)[..., :PWo]
        assert np.array_equal(rows >> 7 != 0, t["dead"]), "bit 7 of the packed mask is not pooled <= 0"
        return host(conv.pool_mask_unpack(mask, T.full((B, 16, PHo, PWo), -2, dtype=T.int32, device="cuda")))

    mask = None
    for prepared in (None, pf):
        what = "prepared" if prepared is not None else "plain"
        pooled, mask = T.full((B, 16, PHo, PWo), 7.0, device="cuda"), new_mask()
        conv.relu_maxpool2_forward(xd, wd, bd, pooled, mask, prepared_fwd=prepared)
        X.bits_equal(host(pooled), t["pooled"], f"pooled ({what})")
        got = as_int32(mask)
        assert np.array_equal(got & 0x7FFFFFFF, t["mask"]), (what, "argmax", int((got & 0x7FFFFFFF != t["mask"]).sum()),
                                                            np.argwhere(got & 0x7FFFFFFF != t["mask"])[:1])
        assert np.array_equal(got < 0, t["dead"]), (what, "mark")
        assert np.array_equal(got, want_mask)
        pooled2 = T.full((B, 16, PHo, PWo), 7.0, device="cuda")
        conv.relu_maxpool2_forward(xd, wd, bd, pooled2, None, prepared_fwd=prepared)  # the no_grad call: no mask
        X.bits_equal(host(pooled2), t["pooled"], f"pooled without a mask ({what})")
    # the gradients read the mask the forward call wrote (equal to the truth's, above)
    new = lambda ref: T.full(ref.shape, 7.0, device="cuda")
    for divisor in (1.0, 4.0):
        gw, gb = new(t["w"]), new(t["b"])
        conv.backward_weight_pooled2(xd, dpool, mask, None, divisor, gw, gb)
        X.bits_equal(host(gw), X.divided(t["S_gw"], divisor), f"pooled-domain gw / {divisor}", 1.0 / divisor)
        X.bits_equal(host(gb), X.divided(t["S_gb"], divisor), f"pooled-domain gb / {divisor}", 1.0 / divisor)
    dx = new(t["x"])
    conv.backward_data_pooled2(dpool, mask, None, wd, dx)
    X.bits_equal(host(dx), t["dx"], "pooled-domain dx")
    dx = new(t["x"])
    conv.backward_data_pooled2(dpool, mask, None, None, dx, prepared_dgrad=pd)
    X.bits_equal(host(dx), t["dx"], "pooled-domain dx (prepared)")
    gw, gb, dx = new(t["w"]), new(t["b"]), new(t["x"])
    conv.backward_pooled2_prepared(xd, dpool, mask, None, pd, 3.0, gw, gb, dx)
    T.cuda.synchronize()
    X.bits_equal(host(dx), t["dx"], "backward_pooled2_prepared dx")
    X.bits_equal(host(gw), X.divided(t["S_gw"], 3.0), "backward_pooled2_prepared gw / 3", 1.0 / 3.0)
    X.bits_equal(host(gb), X.divided(t["S_gb"], 3.0), "backward_pooled2_prepared gb / 3", 1.0 / 3.0)
    if not packed:  # the int32 form also takes the pooled tensor for the ReLU decision instead of the mark
        pooled_d = dev(T, t["pooled"])
        plain_mask = dev(T, t["mask"])
        gw, gb, dx = new(t["w"]), new(t["b"]), new(t["x"])
        conv.backward_weight_pooled2(xd, dpool, plain_mask, pooled_d, 1.0, gw, gb)
        conv.backward_data_pooled2(dpool, plain_mask, pooled_d, wd, dx)
        X.bits_equal(host(gw), X.divided(t["S_gw"], 1.0), "pooled-domain gw (pooled given)")
        X.bits_equal(host(gb), X.divided(t["S_gb"], 1.0), "pooled-domain gb (pooled given)")
        X.bits_equal(host(dx), t["dx"], "pooled-domain dx (pooled given)")
    HELD["first block, pooled domain"] += 1


# ---- 1x1 weight-gradient instances no other test launches ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.C11_CASES, ids=_id)
def test_1x1_wide_channel_instances_are_exact(T, case):
    """c11_wgrad_kernel<3>, <5>, <6> and <7> (conv_1x1.hip: Ci / 16 input-channel groups per workgroup): every call, divisors 1, 3, 4"""
    L, truth, relu_below = _layer(T, case, X.WIDE, 1.0)
    _hold(T, L, _all_calls(T, L), truth, relu_below, None, "default")
    for divisor in (3.0, 4.0):
        L.divisor = divisor
        _hold(T, L, {"backward_weight": R._calls(L, False)["backward_weight"]}, truth, relu_below, None, "default")


@pytest.mark.parametrize("case", X.C11_CASES, ids=_id)
def test_1x1_wide_channel_instances_vs_oracle(T, case):
    """... and on continuous operands against the C oracle, as test_gpu_parity.test_conv2d_mfma_vs_oracle holds its cases"""
    from tests import test_gpu_parity as P

    P.test_conv2d_mfma_vs_oracle(T, case)


# ---- linear -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", X.LINEAR_SHAPES, ids=lambda s: "B%d_%d_%d" % s)
def test_linear_is_exact(T, shape):
    """cnn_linear_forward, cnn_linear_backward (gW, gb, dx; divisors 1 and 4, and 3 on the 25088-input shape), its relu_below form with
    the integer x as the ReLU output below, and the logits of the fused cnn_linear_forward_softmax_xent head (only the logits: the
    softmax goes through expf)"""
    from cnn_amd import capi

    B, n_in, n_out = shape
    x, w, b, dy = X.linear_inputs(B, n_in, n_out, 31)
    x = np.maximum(x, np.float32(0))  # a ReLU layer's output, for both forms: zeros at about half of the positions
    y, S_gw, S_gb, dx = X.linear_truth(x, w, b, dy)
    xd, wd, bd, dyd = dev(T, x), dev(T, w), dev(T, b), dev(T, dy)
    X.bits_equal(host(capi.linear_forward(xd, wd, bd, T.full((B, n_out), 7.0, device="cuda"))), y, "linear y")
    new = lambda *s: T.full(s, 7.0, device="cuda")
    for divisor in (1.0, 4.0) + ((3.0,) if n_in == 25088 else ()):
        for relu in (False, True):
            gw, gb, gdx = capi.linear_backward(xd, dyd, wd, divisor, new(n_in, n_out), new(n_out), new(B, n_in), relu_below=relu)
            what = f"linear, divisor {divisor}{', relu_below' if relu else ''}"
            X.bits_equal(host(gw), X.divided(S_gw, divisor), what + ": gW", 1.0 / divisor)
            X.bits_equal(host(gb), X.divided(S_gb, divisor), what + ": gb", 1.0 / divisor)
            X.bits_equal(host(gdx), np.where(x <= 0, np.float32(0), dx) if relu else dx, what + ": dx")
    HELD["linear entries"] += 1
    if n_out > 8:  # (the fused head covers up to 8 classes)
        return
    labels = dev(T, (np.arange(B) % n_out).astype(np.int32))
    logits, probs, delta, terms = new(B, n_out), new(B, n_out), new(B, n_out), new(B)
    capi.check(capi.load().cnn_linear_forward_softmax_xent(capi._ptr(xd), capi._ptr(wd), capi._ptr(bd), capi._ptr(labels), capi._ptr(logits),
                                                           capi._ptr(probs), capi._ptr(delta), capi._ptr(terms), B, n_in, n_out, capi._stream()),
               "cnn_linear_forward_softmax_xent")
    X.bits_equal(host(logits), y, "logits of the fused loss head")
