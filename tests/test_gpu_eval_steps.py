"""Evaluation in the container (Sequential::eval_begin / eval_step / eval_result) on the device, through cnn_amd.hostapi: the counts,
the predictions and the loss of eval_step are the restatement's (tests/eval_ref.py) on the logits of the same no-grad forward pass, it
launches that pass's kernels plus one, and it changes nothing a train step depends on."""
import numpy as np
import pytest

from cnn_amd import stacks as S
from tests.conv_route_cases import _logged
from tests.eval_ref import ref_accumulate, ref_batch
from tests.util import REL_TOL, assert_close, he_init, uniform01

pytestmark = pytest.mark.gpu

IN = (3, 18, 18)
PLAIN = [("conv", 8, 3, 1, 0), ("relu",), ("pool", 2, 2), ("linear", 3)]
WIDE = [("conv", 8, 3, 1, 0), ("relu",), ("pool", 2, 2), ("linear", 12)]  # more than 8 classes: the unfused loss head's side of the limit
BN_DROP = [("conv", 8, 3, 1, 1), ("bn",), ("relu",), ("dropout", 0.25), ("pool", 2, 2), ("linear", 5)]
SPECS = {"plain": PLAIN, "wide": WIDE, "bn_dropout": BN_DROP}
B = 6
LR = 1e-2
ORACLE_LR = 1e-3  # (the rate of the steps in front of an evaluation that is compared with something)


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def build(which):
    """-> (net, in_shape, classes, name of the logits layer)"""
    from cnn_amd import hostapi

    if which == "alexnet":
        return hostapi.HostAlexNet(3), (3, 224, 224), 3, hostapi._layer_names(S.alexnet(3))[-1]
    spec = SPECS[which]
    net = hostapi.HostSequential(spec, IN)
    return net, IN, net.classes, net.names[-1]


def host_inputs(which, seed, batch=B):
    """-> (p0, x, labels) on the host"""
    spec, in_shape = (S.alexnet(3), (3, 224, 224)) if which == "alexnet" else (SPECS[which], IN)
    layout = S.walk(spec, *in_shape)
    classes = layout[-1]["out"][0]
    x = uniform01(seed + 1, (batch,) + in_shape)
    labels = ((np.arange(batch) * 5 + seed) % classes).astype(np.int32)
    return he_init(layout, seed), x, labels


def inputs(T, which, seed, batch=B):
    """-> (p0, x host, x device, labels host, labels device)"""
    p0, x, labels = host_inputs(which, seed, batch)
    return p0, x, T.from_numpy(x).cuda(), labels, T.from_numpy(labels).cuda()


def no_grad_forward(net, x):
    from cnn_amd import hostapi

    lib = hostapi.load()
    lib.cnnh_set_no_grad(1)
    try:
        return net.forward_host(x)
    finally:
        lib.cnnh_set_no_grad(0)


def check_result(T, got, pred, logits, labels, k, what):
    """counts and predictions exactly the restatement's on these logits; the loss at REL_TOL of the restatement, and bit for bit the
    loss kernel's on the samples whose label is in range"""
    from cnn_amd import capi

    # (the loss kernel's bits are promised while no probability underflows: a spread under 50, include/cnn_amd.h)
    assert np.all(np.isfinite(logits)) and float((logits.max(axis=1) - logits.min(axis=1)).max()) < 50.0, what
    ref = ref_batch(logits, labels, k)
    assert np.array_equal(pred, ref["pred"]), what
    for key in ("samples", "top1", "topk", "ignored"):
        assert got[key] == ref[key], (what, key, got[key], ref[key])
    assert np.array_equal(got["confusion"], ref["confusion"]), what
    print(f"{what}: loss sum {got['loss_sum']!r}, restatement {ref['loss_sum']!r}")
    assert abs(got["loss_sum"] - float(ref["loss_sum"])) <= REL_TOL * abs(float(ref["loss_sum"])), (what, got["loss_sum"], ref["loss_sum"])
    keep = (labels >= 0) & (labels < logits.shape[1])
    if keep.any():
        _, _, loss = capi.softmax_xent(T.from_numpy(np.ascontiguousarray(logits[keep])).cuda(), T.from_numpy(np.ascontiguousarray(labels[keep])).cuda(),
                                       want_probs=False)
        assert np.float64(got["loss_sum"]).tobytes() == (np.float64(0) + np.float64(loss.cpu().numpy()[0])).tobytes(), what
    return ref


@pytest.mark.parametrize("which,k", [("plain", 1), ("wide", 3), ("bn_dropout", 2), ("alexnet", 1)])
def test_eval_step_is_the_no_grad_forward_plus_one_launch(T, which, k):
    net, in_shape, classes, last = build(which)
    batch = 4 if which == "alexnet" else B
    p0, x, xd, labels, ld = inputs(T, which, 40, batch)
    net.set_params(p0)
    for _ in range(2):  # (BatchNorm2D's moving statistics start at mean 0, variance 0: two steps make them a model's)
        net.train_step(xd, ld, ORACLE_LR)
    for _ in range(2):  # (filter images are prepared from the second pass on: both logs are taken in the steady state)
        no_grad_forward(net, x)
    fwd = {}
    log_fwd = _logged(T, lambda: fwd.update(logits=no_grad_forward(net, x)) or {})["log"]
    net.eval_begin(k)

    def step():
        net.eval_step(xd, ld)
        return {}

    log_eval = _logged(T, step)["log"]
    extra = {key: cnt for key, cnt in log_eval.items() if key.split("|")[0].startswith("eval_")}
    rest = {key: cnt for key, cnt in log_eval.items() if key not in extra}
    assert list(extra.values()) == [1], log_eval
    assert rest == log_fwd, (rest, log_fwd)
    pred = net.predictions()
    got = net.eval_result()
    logits = net.layer_output(last, (batch, classes))  # the logits eval_step's kernel read
    assert same(logits, fwd["logits"]), "eval_step's forward pass is the no-grad forward pass"
    check_result(T, got, pred, logits, labels, k, which)
    assert got["accuracy"] == got["top1"] / batch and got["mean_loss"] == got["loss_sum"] / batch
    net.close()


def test_misuse_is_reported(T):
    from cnn_amd import capi

    net, _, _, _ = build("plain")
    _, _, xd, _, ld = inputs(T, "plain", 41)
    for call in (lambda: net.eval_step(xd, ld), net.eval_result, net.predictions, lambda: net.eval_begin(0), lambda: net.eval_begin(4)):
        with pytest.raises(capi.CnnAmdError):
            call()
    net.close()


def snapshot(net):
    m, v, t = net.get_adam_state()
    return {"params": net.get_params(), "grads": net.get_grads(), "velocity": net.get_velocity(), "adam_m": m, "adam_v": v,
            "adam_step": np.asarray([t], np.float32), "accumulator": net.get_accumulated_grads(),
            "phase": np.asarray([net.accumulation_phase()], np.float32), "shadow": net.get_ema(),
            "ema_updates": np.asarray([net.ema_updates()], np.float32)}


def test_eval_has_no_side_effects(T):
    """a BatchNorm2D / Dropout net with Adam state, a velocity arena, an open accumulation window and an average: eval_begin and three
    eval_steps (one on a smaller batch) leave every one of them -- the moving statistics are part of the parameters -- byte-identical"""
    net, _, classes, _ = build("bn_dropout")
    p0, x, xd, labels, ld = inputs(T, "bn_dropout", 42)
    net.set_params(p0)
    net.set_optimizer(0.9, 5e-4)
    net.set_adam(weight_decay=1e-2, decoupled=True)
    net.set_ema(0.9, warmup=True)
    net.set_grad_accumulation(2)
    for _ in range(3):
        net.train_step(xd, ld, 1e-3)
    before = snapshot(net)
    assert before["phase"][0] == 1 and before["ema_updates"][0] == 1 and before["adam_step"][0] == 1
    net.eval_begin(2)
    net.eval_step(xd, ld)
    net.eval_step(xd[:B - 2].contiguous(), ld[:B - 2].contiguous())
    net.eval_step(xd, ld)
    got = net.eval_result()
    assert got["samples"] == 3 * B - 2 and net.predictions().shape == (B,)
    after = snapshot(net)
    for key in before:
        assert same(before[key], after[key]), key
    net.close()


def arm(net, how):
    if how == "adam":
        net.set_adam(weight_decay=1e-2, decoupled=True)
    elif how == "clip":
        net.set_grad_clip(0.5)
    elif how == "accumulation":
        net.set_grad_accumulation(2)


@pytest.mark.parametrize("which,how", [("alexnet", "default"), ("plain", "adam"), ("bn_dropout", "clip"), ("wide", "accumulation")])
def test_twin_nets_agree_when_one_evaluates_in_between(T, which, how):
    """two twins take the same two train steps, one evaluates in between: parameters and last_loss() afterwards are byte-identical.
    "default": the reference net's fused tail, whose pool-fused first block has a deferred data gradient pending when eval_step runs;
    "accumulation": the evaluation falls into the open window"""
    batch = 4 if which == "alexnet" else B
    p0, _, xd, _, ld = inputs(T, which, 43, batch)
    a, b = build(which)[0], build(which)[0]
    for net in (a, b):
        net.set_params(p0)
        arm(net, how)
    if which == "alexnet":  # (the fused tail runs from the second step on: take one more first, so that a data gradient is pending)
        for net in (a, b):
            net.train_step(xd, ld, LR)
    for net in (a, b):
        net.train_step(xd, ld, LR)
    a.eval_begin(1)
    a.eval_step(xd, ld)
    a.eval_step(xd[:batch - 1].contiguous(), ld[:batch - 1].contiguous())
    assert a.eval_result()["samples"] == 2 * batch - 1
    for net in (a, b):
        net.train_step(xd, ld, LR)
    assert same(a.get_params(), b.get_params()), "parameters"
    assert a.last_loss() == b.last_loss() and np.isfinite(a.last_loss())
    assert same(a.get_grads(), b.get_grads()), "gradients"
    a.close()
    b.close()


def test_eval_after_swap_ema_evaluates_the_average(T):
    p0, _, xd, labels, ld = inputs(T, "bn_dropout", 44)
    net, _, classes, last = build("bn_dropout")
    net.set_params(p0)
    net.set_ema(0.5)
    for _ in range(2):
        net.train_step(xd, ld, LR)
    shadow = net.get_ema()
    assert not same(shadow, net.get_params())
    net.swap_ema()
    net.eval_begin(2)
    net.eval_step(xd, ld)
    got, pred = net.eval_result(), net.predictions()
    assert net.ema_swapped(), "eval_step does not swap back"
    logits = net.layer_output(last, (B, classes))
    fresh = build("bn_dropout")[0]
    fresh.set_params(shadow)
    want = fresh.evaluate([(xd, ld)], top_k=2)
    assert same(logits, fresh.layer_output(last, (B, classes))) and np.array_equal(pred, fresh.predictions())
    for key in ("samples", "top1", "topk", "ignored", "loss_sum"):
        assert got[key] == want[key], key
    assert np.array_equal(got["confusion"], want["confusion"])
    check_result(T, got, pred, logits, labels, 2, "averaged")
    net.close()
    fresh.close()


# chosen on the CPU with the oracle alone: every sample separable, three different predictions, the smallest top-two gap 1.4e-3 against 8.5e-4
ORACLE_SEED, ORACLE_B = 45, 8


def oracle_eval_logits(x, labels, p0):
    from oracle import pyoracle as O

    onet = O.SeqNet(BN_DROP, IN)
    onet.params[:] = p0
    for _ in range(2):
        onet.train_step(x, labels, ORACLE_LR)
    return np.asarray(onet.forward(x, training=False), np.float32).reshape(len(labels), -1)


def separable(oev):
    """samples whose prediction the tolerance cannot flip: logits within REL_TOL * max|oracle| of the oracle's, element by element, can
    exchange the two largest only when their gap is at most twice that"""
    top = np.sort(oev, axis=1)
    return (top[:, -1] - top[:, -2]) > 2 * REL_TOL * np.abs(oev).max()


def test_batchnorm_net_agrees_with_the_oracle_in_evaluation_mode(T):
    """after two train steps: the logits eval_step used against oracle.SeqNet's forward(training = False) at REL_TOL (moving statistics,
    Dropout scaling), the predictions wherever the oracle's top-two gap exceeds what that tolerance can flip"""
    p0, x, xd, labels, ld = inputs(T, "bn_dropout", ORACLE_SEED, ORACLE_B)
    net, _, classes, last = build("bn_dropout")
    net.set_params(p0)
    for _ in range(2):
        net.train_step(xd, ld, ORACLE_LR)
    oev = oracle_eval_logits(x, labels, p0)
    net.eval_begin(1)
    net.eval_step(xd, ld)
    pred = net.predictions()
    assert_close(net.layer_output(last, (ORACLE_B, classes)), oev, REL_TOL, "evaluation-mode logits")
    sure = separable(oev)
    assert (~sure).sum() <= ORACLE_B // 4, sure
    assert np.array_equal(pred[sure], np.argmax(oev, axis=1)[sure])
    net.close()


def test_evaluate_over_three_batches_the_last_one_padded(T):
    net, _, classes, _ = build("wide")
    p0, _, _, _, _ = inputs(T, "wide", 46)
    net.set_params(p0)
    batches = []
    for i in range(3):
        _, _, xd, labels, _ = inputs(T, "wide", 47 + i)
        if i == 2:
            labels = labels.copy()
            labels[B - 2:] = -1  # a last batch with two samples of padding
        batches.append((xd, T.from_numpy(labels).cuda()))
    singles = []
    for xd, ld in batches:
        r = net.evaluate([(xd, ld)], top_k=3)
        r["loss_sum"] = np.float32(r["loss_sum"])  # (one call into an empty state: exactly the fp32 batch sum)
        singles.append(r)
    want = ref_accumulate(singles)
    got = net.evaluate(batches, top_k=3)
    assert got["ignored"] == 2 and got["samples"] == 3 * B - 2
    for key in ("samples", "top1", "topk", "ignored"):
        assert got[key] == want[key], key
    assert np.array_equal(got["confusion"], want["confusion"])
    assert np.float64(got["loss_sum"]).tobytes() == np.float64(want["loss_sum"]).tobytes()
    net.close()
