"""architectures::DepthwiseConv2D inside a Sequential (cnn_amd.hostapi.HostSequential) against the oracle's SeqNet on the expanded net.

The net: conv(8,3,2,1) bn relu dwconv(3,1,1) bn relu conv(16,1,1,0) relu dwconv(3,2,1) relu pool(2,2) linear(3) on 3x33x29, and the
three steps once more on 3x32x32: there dw_layer_2 works on 8x16x16 and dw_layer_4 takes 16x16 to 8x8, so the layer's own buffers reach
the 16-byte load / store bodies of the depthwise kernels (17x15 and 9x8 planes stay on the scalar ones).  The
reference is oracle.pyoracle.SeqNet on tests/depthwise_ref.expand_spec (every dwconv as a dense convolution with block-diagonal
filters), its parameters re-expanded from the net's before every step (the dense net's SGD step would fill the off-diagonal zeros), its
gradients and parameters read back through diag_grads.  Batches of 5, 3 (a partial batch) and 5 again; logits, loss, every layer's
gradient block and parameter block after the plain step, once through train_step and once through forward / backward / update.  Then
the container's services on the new layer: checkpoints, the decay and segment tables of Adam and LAMB, layer_output."""
import numpy as np
import pytest

from tests import depthwise_ref as D
from tests import util

pytestmark = pytest.mark.gpu

SPEC = [("conv", 8, 3, 2, 1), ("bn",), ("relu",), ("dwconv", 3, 1, 1), ("bn",), ("relu",), ("conv", 16, 1, 1, 0), ("relu",),
        ("dwconv", 3, 2, 1), ("relu",), ("pool", 2, 2), ("linear", 3)]
IN_SHAPE = (3, 33, 29)
ALIGNED_SHAPE = (3, 32, 32)
BATCHES = (5, 3, 5)
LR = 1e-2


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def _net(in_shape=IN_SHAPE):
    from cnn_amd import hostapi, stacks

    net = hostapi.HostSequential(SPEC, in_shape)
    p0 = stacks.he_init(net.layout, 4242)
    net.set_params(p0)
    return net, p0


def _data(i, B, in_shape=IN_SHAPE):
    x = util.uniform_pm1(8800 + i, (B,) + in_shape)
    labels = ((np.arange(B) + i) % 3).astype(np.int32)
    return x, labels


_REF = {}


def _reference(in_shape=IN_SHAPE):
    """the three steps on the oracle, once per input shape: per step (logits, loss, gradients, parameters after the step, the activation
    of dw_layer_2), all in the depthwise net's own layout"""
    if in_shape not in _REF:
        from cnn_amd import stacks
        from oracle import pyoracle as O

        layout = stacks.walk(SPEC, *in_shape)
        ref = O.SeqNet(D.expand_spec(SPEC), in_shape)
        p = stacks.he_init(layout, 4242)
        steps = []
        for i, B in enumerate(BATCHES):
            ref.params[:] = D.expand_params(layout, p)
            x, labels = _data(i, B, in_shape)
            loss, _ = ref.train_step(x, labels, LR)
            g = D.diag_grads(layout, ref.grads)
            p_new = D.diag_grads(layout, ref.params)
            steps.append(dict(p_before=p, logits=ref.acts[-1].copy(), loss=float(loss), grads=g, params=p_new, dw2=ref.acts[3].copy()))
            p = p_new
        _REF[in_shape] = (steps, layout)
    return _REF[in_shape]


def _blocks(layout):
    off = 0
    for e in layout:
        if e["params"]:
            yield e, off, off + e["params"]
        off += e["params"]


def _close_by_layer(names, layout, got, want, what):
    """every layer's block (weights and bias together: the bias gradient of a convolution in front of a BatchNorm2D is rounding noise
    around an exact zero and is held to the block's scale) at the suite's tolerance"""
    for (e, a, b), name in zip(_blocks(layout), [n for n, e in zip(names, layout) if e["params"]]):
        util.assert_close(got[a:b], want[a:b], util.REL_TOL, what=f"{what}: {name}")


def _three_steps(T, driver, in_shape):
    steps, layout = _reference(in_shape)
    net, _ = _net(in_shape)
    dw2_shape = tuple(layout[3]["out"])
    assert dw2_shape == {IN_SHAPE: (8, 17, 15), ALIGNED_SHAPE: (8, 16, 16)}[in_shape] and layout[3]["kind"] == "dwconv"
    try:
        assert net.names[3] == "dw_layer_2" and net.names[8] == "dw_layer_4" and net.n_params == sum(e["params"] for e in layout)
        for i, (B, want) in enumerate(zip(BATCHES, steps)):
            x, labels = _data(i, B, in_shape)
            xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
            if driver == "train_step":
                net.train_step(xd, ld, LR)
            else:
                net.forward_backward(xd, ld)
                net.update(LR)
            net.flush()
            what = f"{driver} step {i} (B={B})"
            util.assert_close(net.layer_output(net.names[-1], (B, 3)), want["logits"], util.REL_TOL, what=what + ": logits")
            assert abs(net.last_loss() - want["loss"]) < 1e-4 * max(1.0, abs(want["loss"])), (what, net.last_loss(), want["loss"])
            _close_by_layer(net.names, layout, net.get_grads(), want["grads"], what + ": gradient")
            _close_by_layer(net.names, layout, net.get_params(), want["params"], what + ": parameters")
            util.assert_close(net.layer_output("dw_layer_2", (B,) + dw2_shape), want["dw2"], util.REL_TOL, what=what + ": dw_layer_2 output")
    finally:
        net.close()


@pytest.mark.parametrize("driver", ["train_step", "forward_backward_update"])
def test_three_steps_match_the_oracle_on_the_expanded_net(T, driver):
    _three_steps(T, driver, IN_SHAPE)


@pytest.mark.parametrize("driver", ["train_step", "forward_backward_update"])
def test_three_steps_match_the_oracle_on_planes_of_whole_float4_rows(T, driver):
    """3x32x32: 16x16 and 8x8 depthwise planes in the net's own (256-byte aligned) buffers -- the float4 bodies inside a whole step"""
    _three_steps(T, driver, ALIGNED_SHAPE)


def test_checkpoint_round_trip(T, tmp_path):
    from cnn_amd import hostapi

    net, p0 = _net()
    other = hostapi.HostSequential(SPEC, IN_SHAPE)
    try:
        x, labels = _data(0, 5)
        net.train_step(T.from_numpy(x).cuda(), T.from_numpy(labels).cuda(), LR)
        net.flush()
        path = tmp_path / "dw.model"
        net.save_checkpoint(path)
        assert path.stat().st_size == 4 * net.n_params
        before = other.get_params()
        dw_a, dw_b = [(a, b) for e, a, b in _blocks(net.layout) if e["kind"] == "dwconv"][0]
        assert np.abs(before[dw_a:dw_b]).max() > 0  # (the layer initialises itself: Conv2D's scheme)
        other.load_checkpoint(path)
        assert other.get_params().tobytes() == net.get_params().tobytes() != p0.tobytes()
        assert np.fromfile(path, np.float32).tobytes() == net.get_params().tobytes()
    finally:
        net.close()
        other.close()


def _conv_like(layout):
    """the layout as tests/optim_ref.py and tests/lamb_ref.py read it: a dwconv block is weights then C biases, like a convolution's"""
    return [dict(e, kind="conv", Co=e["in"][0]) if e["kind"] == "dwconv" else e for e in layout]


# eps = 1e-3 in both optimizers: the bias gradient of a convolution in front of a BatchNorm2D is rounding noise around an exact zero, and
# with the default eps the first step moves such a parameter by lr * sign(noise) -- a comparison of two roundings, not of two layers
EPS = 1e-3


def test_adam_decays_the_depthwise_weights_and_matches_the_reference_step(T):
    from tests import adam_ref, optim_ref

    steps, layout = _reference()
    want = steps[0]
    for bias_and_norm in (False, True):
        net, p0 = _net()
        try:
            net.set_adam(weight_decay=0.05, decoupled=True, eps=EPS, decay_bias_and_norm=bias_and_norm)
            ranges = optim_ref.decay_ranges_of(_conv_like(layout), bias_and_norm)
            for e, a, b in _blocks(layout):
                if e["kind"] == "dwconv":
                    nw = e["in"][0] * e["k"] ** 2
                    assert any(lo <= a and a + nw <= hi for lo, hi in ranges)                            # the weights decay
                    assert any(lo <= a + nw and b <= hi for lo, hi in ranges) == bias_and_norm           # the bias only on request
            x, labels = _data(0, 5)
            net.forward_backward(T.from_numpy(x).cuda(), T.from_numpy(labels).cuda())
            net.update(1e-3)
            net.flush()
            zeros = np.zeros_like(p0)
            ref_p, _, _ = adam_ref.ref_adam_step(p0, want["grads"], zeros, zeros, 1, 1e-3, eps=EPS, weight_decay=0.05, decoupled=True,
                                                 decay_ranges=ranges)
            moving = optim_ref.moving_stat_mask(layout)
            got = net.get_params()
            _close_by_layer(net.names, layout, np.where(moving, 0, got), np.where(moving, 0, ref_p), f"AdamW step (bias_and_norm={bias_and_norm})")
        finally:
            net.close()


def test_lamb_lists_the_depthwise_tensors_and_matches_the_reference_step(T):
    from tests import lamb_ref, optim_ref

    steps, layout = _reference()
    want = steps[0]
    net, p0 = _net()
    try:
        net.set_lamb(eps=EPS, weight_decay=0.05)
        bounds, flags = net.segment_table()
        rb, rf = lamb_ref.segment_table_of(_conv_like(layout))
        assert np.array_equal(bounds, rb) and np.array_equal(flags, rf)
        for e, a, b in _blocks(layout):
            if e["kind"] == "dwconv":  # weights [C][1][k][k] (decayed, adapted), then bias [C] (neither)
                nw = e["in"][0] * e["k"] ** 2
                i = list(bounds).index(a)
                assert (bounds[i + 1], bounds[i + 2]) == (a + nw, b)
                assert flags[i] == (lamb_ref.SEG_DECAY | lamb_ref.SEG_ADAPT) and flags[i + 1] == 0
        x, labels = _data(0, 5)
        net.forward_backward(T.from_numpy(x).cuda(), T.from_numpy(labels).cuda())
        net.update(1e-3)
        net.flush()
        zeros = np.zeros_like(p0)
        r, _, _ = lamb_ref.ref_lamb_moments(p0, want["grads"], zeros, zeros, bounds, flags, 1, eps=EPS, weight_decay=0.05)
        ref_p = lamb_ref.ref_lamb_step(p0, want["grads"], zeros, zeros, bounds, flags, 1, 1e-3, lamb_ref.ref_segment_norms(p0, bounds),
                                       lamb_ref.ref_segment_norms(r, bounds), eps=EPS, weight_decay=0.05)[0]
        moving = optim_ref.moving_stat_mask(layout)
        _close_by_layer(net.names, layout, np.where(moving, 0, net.get_params()), np.where(moving, 0, ref_p), "LAMB step")
    finally:
        net.close()
