"""Label smoothing, mixup and CutMix through the host classes (Sequential::set_label_smoothing / train_step_mixed / train_step_soft,
cnn_amd.hostapi) on the device: against the oracle (SeqNet.forward -> softmax -> delta = probs - targets -> SeqNet.backward ->
sgd_update on the restatement's mixed batch and targets), the equivalences between the three entries bit for bit, and the launch log:
switched off it is the committed default step, switched on it differs by the head's name and one soft_targets launch."""
import json
import os

import numpy as np
import pytest

from cnn_amd import stacks as S
from tests.soft_target_ref import (MIX_CUTMIX, MIX_MIXUP, PAIR_FLIP, PAIR_NONE, PAIR_ROLL, ref_batch_mix, ref_cutmix_lambda,
                                   ref_soft_targets)
from tests.util import REL_TOL, assert_close, he_init, uniform01

pytestmark = pytest.mark.gpu

SMALL = [("conv", 8, 3, 1, 1), ("relu",), ("pool", 2, 2), ("conv", 16, 3, 2, 0), ("relu",), ("linear", 3)]
SMALL10 = SMALL[:-1] + [("linear", 10)]
SMOOTH = 0.1
LR = 1e-2


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def mix_desc(kind, H, W):
    from cnn_amd import capi

    if kind == "mixup":
        return capi.MixDesc(MIX_MIXUP, 0.3, PAIR_FLIP, 0, 0, 0, 0, 0)
    return capi.MixDesc(MIX_CUTMIX, 0.9, PAIR_ROLL, 1, 2, H // 2 + 1, 1, W // 2 + 3)  # off-centre; its lam field (0.9) must be ignored


def restated(kind, x, labels, classes, smoothing=SMOOTH):
    """the batch and the target rows the step must train on"""
    H, W = x.shape[2:]
    if kind == "smooth":
        return x, ref_soft_targets(labels, classes, smoothing)
    d = mix_desc(kind, H, W)
    box = (d.y0, d.y1, d.x0, d.x1)
    lam = d.lam if kind == "mixup" else ref_cutmix_lambda(H, W, *box)
    return ref_batch_mix(x, d.mode, d.lam, d.pair_rule, d.pair_shift, box), ref_soft_targets(labels, classes, smoothing, lam, d.pair_rule, d.pair_shift)


def step(net, kind, xd, ld, lr=LR):
    if kind == "smooth":
        net.train_step(xd, ld, lr)
    else:
        net.train_step_mixed(xd, ld, lr, mix_desc(kind, xd.shape[2], xd.shape[3]))


def against_oracle(T, spec, in_shape, B, kinds, seed, net=None):
    """one step per entry of `kinds`: loss, target rows, gradients and parameters against the oracle on the restatement's batch and
    targets; the oracle takes its ReLU / pool decisions from the device's forward tensors (masks_from, as tests/test_gpu_stacks.py) and
    starts every step from the device's parameters"""
    from cnn_amd import hostapi
    from oracle import pyoracle as O

    onet = O.SeqNet(spec, in_shape)
    classes = onet.layers[-1]["out"][0]
    p0 = he_init(onet.layers, seed)
    x = uniform01(seed + 1, (B,) + in_shape)
    labels = ((np.arange(B) * 2 + 1) % classes).astype(np.int32)
    xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    net = net or hostapi.HostSequential(spec, in_shape)
    names = hostapi._layer_names(spec)
    net.set_params(p0)
    net.set_label_smoothing(SMOOTH)
    for n, kind in enumerate(kinds):
        xm, targets = restated(kind, x, labels, classes)
        onet.params[:] = net.get_params()
        p_before = onet.params.copy()
        step(net, kind, xd, ld)
        assert same(net.last_targets(B), targets), (kind, "target rows")
        probs = O.softmax(onet.forward(xm))
        with np.errstate(divide="ignore"):
            oloss = float(-(targets.astype(np.float64) * np.log(probs.astype(np.float64))).sum() / B)
        loss = net.last_loss()
        assert abs(loss - oloss) <= REL_TOL * max(1.0, abs(oloss)), (kind, loss, oloss)
        masks = {}
        for idx, e in enumerate(onet.layers):
            if e["kind"] == "relu":
                masks[idx] = net.layer_output(names[idx], (B,) + e["out"])
                if idx + 1 < len(onet.layers) and onet.layers[idx + 1]["kind"] == "pool":
                    masks[idx + 1] = masks[idx]
        onet.backward((probs - targets).astype(np.float32), masks_from=masks)
        g = net.get_grads()
        for e in onet.layers:
            if e.get("n", 0) > 0:
                sl = slice(e["off"], e["off"] + e["n"])
                assert_close(g[sl], onet.grads[sl], REL_TOL, f"step {n} {kind}: {e['kind']} gradients")
        assert_close(net.get_params(), O.sgd_update(p_before, onet.grads, LR), REL_TOL, f"step {n} {kind}: parameters")
    net.close()


@pytest.mark.parametrize("spec", [SMALL, SMALL10], ids=["linear3_fused_head", "linear10_generic_head"])
def test_small_net_against_the_oracle(T, spec):
    """3 x 25 x 25, B = 5 (FLIP pairs the middle sample with itself): two steps each of train_step under smoothing, train_step_mixed in
    MIXUP (lam 0.3, FLIP) and in CUTMIX (an off-centre box, ROLL 1)"""
    against_oracle(T, spec, (3, 25, 25), 5, ["smooth", "smooth", "mixup", "mixup", "cutmix", "cutmix"], 810)


def test_reference_net_against_the_oracle(T):
    """the reference net at B = 4: pool-fused first block, fused step tail, the register-resident in = 4608 head; three steps"""
    from cnn_amd import hostapi

    against_oracle(T, S.alexnet(3), (3, 224, 224), 4, ["mixup", "cutmix", "smooth"], 820, net=hostapi.HostAlexNet(3))


def _alexnet_inputs(T, B, seed):
    layout = S.walk(S.alexnet(3), 3, 224, 224)
    p0 = he_init(layout, seed)
    x = uniform01(seed + 1, (B, 3, 224, 224))
    labels = ((np.arange(B) + 1) % 3).astype(np.int32)
    return p0, x, labels


@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_mixed_step_equals_soft_step_on_the_premixed_batch(T, kind):
    """train_step_mixed(x, labels, mix) on one net, train_step_soft(cnn_batch_mix(x), cnn_soft_targets(labels, ...)) on its twin, three
    steps: parameters, gradients, loss and the input delta bit for bit; the first layer's get_output() re-computes from the MIXED batch"""
    from cnn_amd import capi, hostapi

    B = 4
    p0, x, labels = _alexnet_inputs(T, B, 830)
    xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    d = mix_desc(kind, 224, 224)
    lam = d.lam if kind == "mixup" else capi.cutmix_lambda(224, 224, d.y0, d.y1, d.x0, d.x1)
    xm = capi.batch_mix(d, xd)
    targets = capi.soft_targets(ld, 3, SMOOTH, lam, d.pair_rule, d.pair_shift)
    a, b = hostapi.HostAlexNet(3), hostapi.HostAlexNet(3)
    for net in (a, b):
        net.set_params(p0)
    a.set_label_smoothing(SMOOTH)
    for n in range(3):
        a.train_step_mixed(xd, ld, LR, d)
        b.train_step_soft(xm, targets, LR)
        assert a.last_loss() == b.last_loss() and np.isfinite(a.last_loss()), n
        assert same(a.get_params(), b.get_params()), (n, "parameters")
        assert same(a.get_grads(), b.get_grads()), (n, "gradients")
        assert same(a.input_delta(x.shape), b.input_delta(x.shape)), (n, "input delta")
        assert same(a.last_targets(B), b.last_targets(B)) and same(a.last_targets(B), targets.cpu().numpy())
    shape = (B, 16, 111, 111)
    out_a = a.layer_output("conv_layer_1", shape)
    assert same(out_a, b.layer_output("conv_layer_1", shape))
    c = hostapi.HostAlexNet(3)  # ... and not from the batch the caller passed
    c.set_params(p0)
    for n in range(3):
        c.train_step_soft(xd, targets, LR)
    assert not same(out_a, c.layer_output("conv_layer_1", shape))
    for net in (a, b, c):
        net.close()


def test_back_to_back_mixed_steps_equal_flushed_ones(T):
    """three mixed steps with nothing in between -- the next step's mix rewrites the container's mixed batch while the previous step's
    deferred work may still be queued -- against the same three with flush() after each, then a partial batch of 3"""
    from cnn_amd import hostapi

    B = 4
    p0, x, labels = _alexnet_inputs(T, B, 840)
    xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    kinds = ["mixup", "cutmix", "mixup"]
    a, b = hostapi.HostAlexNet(3), hostapi.HostAlexNet(3)
    for net in (a, b):
        net.set_params(p0)
        net.set_label_smoothing(SMOOTH)
    for kind in kinds:
        step(a, kind, xd, ld)
    for kind in kinds:
        step(b, kind, xd, ld)
        b.flush()
        T.cuda.synchronize()
    assert same(a.get_params(), b.get_params()) and same(a.get_grads(), b.get_grads()) and a.last_loss() == b.last_loss()
    step(a, "mixup", xd[:3], ld[:3])
    step(b, "mixup", xd[:3], ld[:3])
    b.flush()
    assert same(a.get_params(), b.get_params()) and same(a.get_grads(), b.get_grads()) and a.last_loss() == b.last_loss()
    xm, targets = restated("mixup", x[:3], labels[:3], 3)
    assert same(a.last_targets(3), targets)
    a.close()
    b.close()


def _step_kernels(T, net, x, labels, steps=3):
    from cnn_amd import capi

    T.cuda.synchronize()
    capi.kernel_timing(0)
    capi.kernel_timing_report()  # (records an earlier test left behind are not this net's launches)
    capi.kernel_timing(1)
    for _ in range(steps):
        net.train_step(x, labels, 1e-3)
    net.flush()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    return {k: cnt for k, (cnt, _) in rep.items()}


def test_smoothing_off_is_the_default_path(T, golden_dir):
    """after set_label_smoothing(0.1) and set_label_smoothing(0) three train_steps of a fresh reference net launch exactly the committed
    golden list and end with a never-armed net's parameters.  With smoothing on, the log differs from the golden one by the head's name
    and one soft_targets launch per step, and nothing else."""
    from tests.test_gpu_optimizer import make_net, net_inputs

    layout, p0, x, labels = net_inputs(T, "alexnet", 340)
    golden = json.load(open(os.path.join(golden_dir, "train_step_kernels_before_optimizer.json")))
    runs = {}
    for mode in ("never", "off_again", "on"):
        net = make_net("alexnet")
        net.set_params(p0)
        if mode != "never":
            net.set_label_smoothing(0.1)
        if mode == "off_again":
            net.set_label_smoothing(0)
        runs[mode] = (_step_kernels(T, net, x, labels), net.get_params())
        net.close()
    assert runs["off_again"][0] == golden, sorted(set(runs["off_again"][0].items()) ^ set(golden.items()))
    assert runs["never"][0] == golden and same(runs["never"][1], runs["off_again"][1])
    on = runs["on"][0]
    hard_heads = {k: c for k, c in golden.items() if k.startswith("linear_fwd+softmax_xent")}
    assert hard_heads and not any(k.startswith(("soft_targets", "linear_fwd+softmax_xent_soft")) for k in golden)
    renamed = {k.replace("linear_fwd+softmax_xent", "linear_fwd+softmax_xent_soft"): c for k, c in hard_heads.items()}
    extra = {k: c for k, c in on.items() if k.startswith("soft_targets")}
    assert len(extra) == 1 and sum(extra.values()) == 3, extra
    want = {k: c for k, c in golden.items() if k not in hard_heads}
    want.update(renamed)
    want.update(extra)
    assert on == want, sorted(set(on.items()) ^ set(want.items()))
    assert not same(runs["on"][1], runs["never"][1])


def test_smoothed_steps_under_clipping_accumulation_and_the_average(T):
    """the route does not depend on the targets: with clipping, accumulation (k = 2) and the average on -- the plain sequence --
    train_step under smoothing equals train_step_soft on the same rows, bit for bit, and forward_backward leaves the same gradients as
    the first micro-batch"""
    from cnn_amd import capi, hostapi

    B = 4
    p0, x, labels = _alexnet_inputs(T, B, 850)
    xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    targets = capi.soft_targets(ld, 3, SMOOTH)
    a, b, c = hostapi.HostAlexNet(3), hostapi.HostAlexNet(3), hostapi.HostAlexNet(3)
    for net in (a, b):
        net.set_params(p0)
        net.set_adam(weight_decay=1e-2, decoupled=True)
        net.set_grad_clip(0.5)
        net.set_grad_accumulation(2)
        net.set_ema(0.9)
    a.set_label_smoothing(SMOOTH)
    c.set_params(p0)
    c.set_label_smoothing(SMOOTH)
    c.forward_backward(xd, ld)
    for n in range(4):
        a.train_step(xd, ld, 1e-3)
        b.train_step_soft(xd, targets, 1e-3)
        if n == 0:
            assert same(a.get_grads(), c.get_grads()) and a.last_loss() == c.last_loss()
        assert a.last_loss() == b.last_loss() and same(a.get_params(), b.get_params()) and same(a.get_grads(), b.get_grads()), n
    assert same(a.get_ema(), b.get_ema()) and not same(a.get_params(), p0)
    for net in (a, b, c):
        net.close()
