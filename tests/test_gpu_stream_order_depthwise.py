"""Stream order of the entry points that serve CNN_CONV2D_DEPTHWISE (tests/stream_order.py is the harness; the flag adds no export, so
tests/test_stream_order_coverage.py has nothing new to place): the three passes and cnn_conv2d_backward, one 3x3 case and one generic
case, caller late -- behind a gated stream with x, w, bias, dy and relu_below arriving late and the workspace poisoned -- and the fork /
join calls helper late, with the gate on the library's side stream.  The reference is the lattice truth of tests/depthwise_ref.py (one
correct bit pattern per element), and the gated run must give the bits of the plain run."""
import numpy as np
import pytest

from tests import depthwise_calls as DC
from tests import depthwise_ref as D
from tests import exact as X
from tests import stream_order as SO

pytestmark = pytest.mark.gpu

CASES = [D.K3_S2[2], D.GENERIC[0]]  # (3, 33, 14, 14, 3, 2, 1) and (2, 3, 11, 12, 5, 1, 2)
DIVISOR = 4.0


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture
def H(T):
    h = SO.harness(T)
    try:
        yield h
    finally:
        h.finish()


def _want(case):
    (x, w, b, dy, below), (y, S_gw, S_gb, dx) = D.lattice_case(case)
    return {"y": y, "y_relu": np.maximum(y, np.float32(0)), "dx": dx, "dx_masked": np.where(below <= 0, np.float32(0), dx),
            "gw": X.divided(S_gw, DIVISOR), "gb": X.divided(S_gb, DIVISOR)}


def _calls(L):
    return {"forward": L.forward, "forward_relu": L.forward_relu, "backward_data": L.backward_data, "backward_data_relu": L.backward_data_relu,
            "backward_weight": lambda: L.backward_weight(DIVISOR), "backward/join": lambda: L.backward(DIVISOR, 0),
            "backward/defer": lambda: L.backward(DIVISOR, 1), "backward_weight_side": lambda: L.backward_weight(DIVISOR, side=True)}


def _hold(res, want, what):
    assert not isinstance(res.gated, int), (what, res.gated)
    for name, a in res.gated.items():
        X.bits_equal(a, want[name], f"{what}: {name} (gated)")
    res.assert_same_bits_as_plain(what)


@pytest.mark.parametrize("case", CASES, ids=D.key)
def test_depthwise_calls_caller_late(T, H, case):
    L = DC.Layer(T, case, D.lattice_case(case)[0], guard_outputs=False)
    T.cuda.synchronize()
    late = [H.late(getattr(L, name), 9700 + j) for j, name in enumerate(("x", "w", "b", "dy", "below"))]
    want = _want(case)
    for name, fn in _calls(L).items():
        what = f"depthwise {D.key(case)}:{name}"
        _hold(H.caller_late(what, late, fn, poison=[L.ws.view]), want, what)


@pytest.mark.parametrize("case", CASES, ids=D.key)
def test_depthwise_fork_and_join_helper_late(T, H, case):
    """the gate on the library's side stream: the weight gradient waits there, the join the contract names orders it in front of the clones"""
    L = DC.Layer(T, case, D.lattice_case(case)[0], guard_outputs=False)
    T.cuda.synchronize()
    want = _want(case)
    calls = _calls(L)
    for name in ("backward/join", "backward/defer", "backward_weight_side"):
        what = f"depthwise {D.key(case)}:{name} (helper late)"
        _hold(H.helper_late(what, calls[name], poison=[L.ws.view]), want, what)
