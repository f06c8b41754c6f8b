"""Stream order of the Python driver (cnn_amd/pynet.py; tests/stream_order.py is the harness): three train steps and flush() of
AlexNetHip(2, 3) on S -- in the default configuration and with the conv 1 data gradient deferred onto side_b, the pool-fused first
block and the early SGD step on the library's side stream -- caller late (batch, labels and parameters arrive late) and helper late
(side_b / the library's side stream gated), against the CPU oracle's three steps."""
import numpy as np
import pytest

from tests import stream_order as SO
from tests.util import REL_TOL, assert_close, normal_scaled, uniform01

pytestmark = pytest.mark.gpu

B, LR, STEPS = 2, 1e-3, 3
CONFIGS = {"default": {}, "deferred_pool_fused": dict(defer_input_grad=True, fuse_pool=True)}
# Three whole train steps are queued behind one gate: 0.8 ms of host time (measured: profiles/stream_order.md), a twenty-fifth of
# the harness's default gate.
GATE_MS = SO.GATE_MS


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


def inputs():
    from oracle import pyoracle as O

    return {"x": uniform01(7900, (B, 3, 224, 224)), "labels": np.array([0, 2], np.int32), "params": normal_scaled(7901, (O.Net(B, 3).n_params,))}


def decoys():
    """another batch, every label wrong, another initialisation of the same scale (finite steps, far from the real ones)"""
    real = inputs()
    return {"x": SO.decoy_of(real["x"], 7911), "labels": ((real["labels"] + 1) % 3).astype(np.int32), "params": normal_scaled(7912, real["params"].shape)}


def oracle_steps(inp):
    """-> {params, logits, loss_sum, d_conv0} after STEPS steps of the CPU oracle (the last step's logits, loss and input delta)"""
    from oracle import pyoracle as O

    onet = O.Net(B, 3)
    onet.params[:] = inp["params"]
    for _ in range(STEPS):
        logits = onet.forward(inp["x"])
        loss, delta = O.cross_entropy_backward(O.softmax(logits), inp["labels"])
        onet.backward(delta)
        d0 = onet.d_conv(0).copy()
        onet.update(LR)
    return {"params": onet.params.copy(), "logits": logits.copy(), "loss_sum": np.array([loss * B], np.float32), "d_conv0": d0}


@pytest.fixture(scope="module")
def reference():
    return oracle_steps(inputs())


def _tensors_of(T, obj):
    out = []
    for v in vars(obj).values():
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            for u in (t if isinstance(t, (list, tuple)) else [t]):
                if isinstance(u, T.Tensor):
                    out.append(u)
    return out


# (side_b exists only with the deferred conv 1 data gradient)
PLACEMENTS = [("default", "caller_late"), ("default", "helper_late_side_stream"), ("deferred_pool_fused", "caller_late"),
              ("deferred_pool_fused", "helper_late_side_b"), ("deferred_pool_fused", "helper_late_side_stream")]


@pytest.mark.parametrize("config,placement", PLACEMENTS, ids=["-".join(p) for p in PLACEMENTS])
def test_python_driver_steps(T, H, reference, config, placement):
    from cnn_amd.pynet import AlexNetHip

    net = AlexNetHip(B, 3, **CONFIGS[config])
    if config == "deferred_pool_fused":
        assert net.fuse_pool and net.defer_dx0 and net.early_update
    inp = inputs()
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, ld, p0 = dev(inp["x"]), dev(inp["labels"]), dev(inp["params"])
    # every buffer the driver owns is poisoned (activations, deltas, gradients, prepared filters, workspaces): what the ungated run
    # left there are the right values of the very same steps
    inputs_of_the_steps = {t.data_ptr() for t in (xd, ld, p0, net.params)}  # (net.x is the batch once a step has run)
    poison = [t for t in _tensors_of(T, net) if t.data_ptr() not in inputs_of_the_steps] + [c.ws for c in net.convs]
    T.cuda.synchronize()
    dec = decoys()
    late = [H.late(xd, 0, decoy=dev(dec["x"])), H.late(ld, 0, decoy=dev(dec["labels"])), H.late(net.params, 0, real=p0, decoy=dev(dec["params"]))]

    def call():
        net.params.copy_(p0)
        net._prep_valid = False
        for _ in range(STEPS):
            net.train_step(xd, ld, LR)
        net.flush()
        return {"params": net.params, "logits": net.logits, "loss_sum": net.loss_sum, "d_conv0": net.d_conv[0]}

    what = f"pynet {config} {placement}"
    if placement == "caller_late":
        res = H.caller_late(what, late, call, poison=poison, gate_ms=GATE_MS)
    else:
        res = H.helper_late(what, call, helper=net.side_b if placement.endswith("side_b") else H.side, poison=poison, gate_ms=GATE_MS)
    assert_close(res.gated["params"], reference["params"], REL_TOL, f"{what}: params after {STEPS} steps")
    assert_close(res.gated["logits"], reference["logits"], REL_TOL, f"{what}: logits of the last step")
    assert np.isclose(res.gated["loss_sum"][0] / B, reference["loss_sum"][0] / B, rtol=1e-4), what
    assert_close(res.gated["d_conv0"], reference["d_conv0"], REL_TOL, f"{what}: input delta of the last step")
    res.assert_same_bits_as_plain(what)
