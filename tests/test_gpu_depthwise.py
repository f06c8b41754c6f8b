"""CNN_CONV2D_DEPTHWISE through the C ABI on guarded buffers (tests/depthwise_calls.py, tests/guarded.py).

Exact bits on the integer lattice (tests/exact.py, tests/depthwise_ref.py: one correct fp32 pattern per element of y, relu(y), dx, the
masked dx, gw and gb), the suite's tolerance against the C oracle on block-diagonal filters for continuous operands, which kernel ran
(the dw_* names of the kernel-timing report: the specialised 3x3 kernels for k = 3 and stride 1 / 2, the generic ones otherwise, never
a dense family), the slab planner's branches (CUS), cnn_conv2d_backward with both defer_join values and the weight gradient on the
side stream, and that a depthwise call leaves the routes and results of flag-free descs in the same process alone.  Every case runs
once more with x, dy and w moved off every 16-byte boundary (the scalar-load bodies of the same kernels).

Which body ran: a 3x3 launch picks its row loads (dw_load_row<NW, OFF>, OFF in {0, 1, 2, -1}; PP for the stride-2 data gradient) and
float4 or scalar stores / mask reads / dy loads from widths, padding and pointer alignment, and says so behind the geometry tag of its
kernel-timing key.  depthwise_ref.VARIANT_CASES x SHIFT_ROWS launch all 34 reachable combinations (proven on the CPU in
tests/test_depthwise_reference.py); every launch here must carry the variant depthwise_ref.launch_variants names for it."""
import numpy as np
import pytest

from tests import conv_route_cases as R
from tests import depthwise_calls as DC
from tests import depthwise_ref as D
from tests import exact as X
from tests import util

pytestmark = pytest.mark.gpu

DENSE_NAMES = ("igemm", "conv_rows", "rows_", "conv_1x1", "conv_direct", "fwd_rd", "dgrad_rd", "wgrad_kernel", "wgrad_rd", "wgrad_sp", "conv_wgrad",
               "conv_stem", "thin", "pk_", "im2col", "bias_grad")


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    arch = capi.load().cnn_amd_device_arch().decode()
    assert arch == "gfx950", f"built for gfx950, running on {arch}"
    return torch


def _want_lattice(truth, below, divisor):
    y, S_gw, S_gb, dx = truth
    return {"y": (y, 1.0), "y_relu": (np.maximum(y, np.float32(0)), 1.0), "dx": (dx, 1.0),
            "dx_masked": (np.where(below <= 0, np.float32(0), dx), 1.0),
            "gw": (X.divided(S_gw, divisor), 1.0 / divisor), "gb": (X.divided(S_gb, divisor), 1.0 / divisor)}


def _all_calls(L, divisor):
    """name -> thunk of every call that serves the flag"""
    return {"forward": L.forward, "forward_relu": L.forward_relu, "forward_relu/only": lambda: L.forward_relu(with_y=False),
            "backward_data": L.backward_data, "backward_data_relu": L.backward_data_relu,
            "backward_weight": lambda: L.backward_weight(divisor)}


def _expected_kernels(case, call):
    B, C, H, W, k, s, pad = case
    spec = k == 3 and s in (1, 2)
    tag = f"<3x3,s{s}>" if spec else "<generic>"
    if call.startswith("forward"):
        return ["dw_fwd" + tag]
    if call.startswith("backward_data"):
        return ["dw_dgrad" + tag]
    return ["dw_wgrad" + tag, "slab_reduce/final"]


def _hold_exact(T, case, lattice, divisor, shift_bytes, calls=None, check_kernels=True):
    """shift_bytes: one number (x, dy and w moved by it) or a row of depthwise_ref.SHIFT_ROWS"""
    (x, w, b, dy, below), truth = D.lattice_case(case, lattice)
    row = shift_bytes if isinstance(shift_bytes, tuple) else (shift_bytes, shift_bytes, 0, 0)
    L = DC.Layer(T, case, (x, w, b, dy, below), shifts=D.shifts_of(row))
    want = _want_lattice(truth, below, divisor)
    model = D.launch_variants(case, L.shifts)
    wrong = []
    for name, fn in (calls(L) if calls else _all_calls(L, divisor)).items():
        out, keys = DC.logged(T, fn, keys=True)
        names = [k.split("|")[0] for k in keys]
        if check_kernels and names != _expected_kernels(case, name):
            wrong.append(f"{name}: launched {names}, expected {_expected_kernels(case, name)}")
        for k in keys:  # the body the launch chose is the one the model names (for this call where it is one of D.CALLS)
            if model and k.startswith("dw_"):
                got = D.tag_variant(k)
                if got is None or (got != model[name] if name in model else got not in set(model.values())):
                    wrong.append(f"{name}: {k} is variant {got}, the model says {model.get(name, sorted(set(model.values())))}")
        if any(d in n for n in names for d in DENSE_NAMES):
            wrong.append(f"{name}: a dense family ran: {names}")
        for o, t in sorted(out.items()):
            report = X.bits_differ(DC.host(t), want[o][0], f"{name}: {o}", want[o][1])
            if report:
                wrong.append(report)
    wrong += L.intact()
    assert not wrong, f"{D.key(case)} amp{lattice[0]} shift {shift_bytes}:\n" + "\n".join(wrong)


def _runs():
    return [(c, X.WIDE) for c in D.ODD_WIDTH_CASES] + [(c, X.NARROW) for c in D.NARROW_CASES]


@pytest.mark.parametrize("shift_bytes", [0, 4], ids=["aligned", "shift4"])
@pytest.mark.parametrize("case,lattice", _runs(), ids=lambda v: D.key(v) if len(v) > 2 else "amp%d" % v[0])
def test_every_pass_is_exact_and_runs_its_kernel(T, case, lattice, shift_bytes):
    """y, relu(y) (with and without y), dx, the masked dx, gw and gb (divisor 4: exact) bit for bit; the kernel of every pass by name"""
    _hold_exact(T, case, lattice, 4.0, shift_bytes)


@pytest.mark.parametrize("row", D.SHIFT_ROWS, ids=D.shift_key)
@pytest.mark.parametrize("case", D.VARIANT_CASES, ids=D.key)
def test_every_load_and_store_variant_is_exact_and_is_the_one_the_model_names(T, case, row):
    """widths that are multiples of 4, pads 0..4 and every operand group on and off the 16-byte boundary: the float4 bodies of the row
    loads, the stores, the mask read and the dy load, bit for bit in every pass, each launch tagged with the variant the model names"""
    _hold_exact(T, case, X.WIDE, 4.0, row)


@pytest.mark.parametrize("row", D.SHIFTS_BOTH, ids=D.shift_key)
@pytest.mark.parametrize("case", D.VARIANT_NARROW_CASES, ids=D.key)
def test_float4_bodies_are_exact_on_the_narrow_lattice(T, case, row):
    _hold_exact(T, case, X.NARROW, 4.0, row)


@pytest.mark.parametrize("case", [D.K3_S1[2], D.K3_S2[2], D.GENERIC[0], D.VARIANT_S1[2], D.VARIANT_S2[0]], ids=D.key)
def test_weight_gradient_is_the_rounded_quotient(T, case):
    """divisor 3: the correctly rounded quotient of the exact sum, which sum * (1 / 3) or a division per slab does not give"""
    _hold_exact(T, case, X.WIDE, 3.0, 0, calls=lambda L: {"backward_weight": lambda: L.backward_weight(3.0)})


@pytest.mark.parametrize("shift_bytes", [0, 4], ids=["aligned", "shift4"])
@pytest.mark.parametrize("case", D.CASES, ids=D.key)
def test_every_pass_matches_the_oracle_on_continuous_operands(T, case, shift_bytes):
    """util.normal_scaled filters, the C oracle on expand_filters(w), the suite's REL_TOL"""
    ins, (y, gw, gb, dx) = D.continuous_case(case)
    L = DC.Layer(T, case, ins, shift_bytes)
    below = ins[4]
    want = {"y": y, "y_relu": np.maximum(y, np.float32(0)), "dx": dx, "dx_masked": np.where(below <= 0, np.float32(0), dx), "gw": gw, "gb": gb}
    for name, fn in _all_calls(L, float(case[0])).items():
        for o, t in fn().items():
            util.assert_close(DC.host(t), want[o], util.REL_TOL, what=f"{D.key(case)} {name}: {o}")
    assert not L.intact()


def test_forward_relu_and_masked_gradient_equal_the_separate_calls(T):
    """bit-identical to forward + cnn_relu_forward and to the data gradient + cnn_relu_backward, on continuous operands"""
    from cnn_amd import capi

    for case in (D.K3_S1[3], D.K3_S2[3], D.GENERIC[1]):
        ins, _ = D.continuous_case(case)
        L = DC.Layer(T, case, ins)
        y = L.forward()["y"]
        fused = L.forward_relu()
        assert T.equal(fused["y"], y) and T.equal(fused["y_relu"], capi.relu_forward(y.clone()))
        assert T.equal(L.forward_relu(with_y=False)["y_relu"], fused["y_relu"])
        dx = L.backward_data()["dx"].clone()
        capi.check(capi.load().cnn_relu_backward(capi._ptr(L.below), capi._ptr(dx), dx.numel(), capi._stream()), "cnn_relu_backward")
        assert T.equal(L.backward_data_relu()["dx_masked"], dx)
        assert not L.intact()


@pytest.mark.parametrize("cus", ["2", "1000"])
@pytest.mark.parametrize("case", D.LARGEST, ids=D.key)
def test_largest_cases_give_the_same_bits_at_other_cu_counts(T, lib_option, case, cus):
    """the two largest cases with the planner told the card has 2 compute units and more than it has"""
    lib_option("CUS", cus)
    _hold_exact(T, case, X.WIDE, 4.0, 0)
    lib_option("CUS", None)
    _hold_exact(T, case, X.WIDE, 4.0, 0)


@pytest.mark.parametrize("cus,slabs", [("1", 2), ("2", 3), (None, 6)])
@pytest.mark.parametrize("case", [(6, 3, 9, 9, 3, 1, 1), (6, 3, 11, 12, 5, 1, 2), (6, 3, 8, 8, 3, 1, 1)], ids=D.key)
def test_slab_planner_branches_give_the_same_bits(T, lib_option, case, cus, slabs):
    """six samples of three channels: the planner (four workgroups per compute unit over the channels) makes two slabs of three samples
    at CUS=1, three of two at CUS=2 and one per sample on the whole card -- seen in the workspace size -- and the bits do not move
    (9x9: the scalar bodies of dw3_wgrad, 8x8: its float4 row and dy loads)"""
    import ctypes as C

    from cnn_amd import capi

    lib_option("CUS", cus)
    B, Cn, H, W, k, s, pad = case
    d = capi.ConvDesc(B, Cn, H, W, Cn, k, s, pad, capi.DEPTHWISE)
    assert int(capi.load().cnn_conv2d_workspace_bytes(C.byref(d))) == ((slabs + 1) * Cn * (k * k + 1) + 64) * 4
    _hold_exact(T, case, X.WIDE, 4.0, 0, calls=lambda L: {"backward_weight": lambda: L.backward_weight(4.0),
                                                          "backward_weight/3": lambda: L.backward_weight(4.0)})


@pytest.mark.parametrize("case", [D.K3_S1[3], D.K3_S2[2], D.GENERIC[1], D.VARIANT_S1[2]], ids=D.key)
def test_backward_in_one_call_equals_the_separate_calls(T, case):
    """cnn_conv2d_backward with defer_join 0 and 1 (join, then compare) and cnn_conv2d_backward_weight_side: the bits of the separate calls"""
    def calls(L):
        return {"backward/join": lambda: L.backward(4.0, 0), "backward/defer": lambda: L.backward(4.0, 1),
                "backward_weight_side": lambda: L.backward_weight(4.0, side=True)}

    _hold_exact(T, case, X.WIDE, 4.0, 0, calls=calls, check_kernels=False)
    (x, w, b, dy, below), _ = D.continuous_case(case)
    L = DC.Layer(T, case, (x, w, b, dy, below))
    sep = dict(L.backward_weight(float(case[0])), **L.backward_data())
    for defer in (0, 1):
        (got, names) = DC.logged(T, lambda: L.backward(float(case[0]), defer))
        assert all(T.equal(got[o], sep[o]) for o in ("gw", "gb", "dx")), (defer, names)
        assert sum(n.startswith("dw_wgrad") for n in names) == 1 and sum(n.startswith("dw_dgrad") for n in names) == 1, names
    assert not L.intact()


def test_dense_routes_are_untouched_by_a_depthwise_call(T):
    """three flag-free descs of tests/conv_route_cases.py and the dense twin of a depthwise case: kernel names and output bits before and
    after depthwise calls of the same geometry in the same process are identical (the RouteFacts / DescMemo rings key on the flags)"""
    HP = R.HAND_PICKED
    dw_case = D.K3_S1[3]                                  # (2, 40, 14, 14, 3, 1, 1)
    cases = [HP[13], HP[5], HP[26], D.dense_case(dw_case)]
    layers = [R._Layer(T, c, 9300 + i) for i, c in enumerate(cases)]
    names = ("forward", "forward_relu", "backward_data", "backward_data_relu", "backward_weight")

    def record():
        return [{n: R._logged(T, R._calls(L, False)[n]) for n in names} for L in layers]

    before = record()
    for rec in before:
        assert all("sha" in r and not any(k.startswith("dw_") for k in r["log"]) for r in rec.values()), rec
    for case in (dw_case, (2, 32, 14, 14, 3, 1, 1), (2, 64, 7, 7, 1, 1, 0)):  # ... and the twins of HP[13] (Co != Ci) and HP[5] by B, Ci, H, W
        L = DC.Layer(T, case, D.lattice_case(case)[0])
        for fn in _all_calls(L, 4.0).values():
            out, log = DC.logged(T, fn)
            assert log and all(n.startswith(("dw_", "slab_reduce")) for n in log), log
    assert record() == before
