"""The exponential moving average of the parameters in the container (Sequential::set_ema / swap_ema / save_ema_state) on the device,
through cnn_amd.hostapi.  The shadow is held bit for bit to the NumPy restatement (tests/ema_ref.py) applied to the parameters the
device reports after every step; the average moves no parameter, launches one kernel per optimizer step, swaps in and out of the
arena without losing a bit, and survives a state file."""
import json
import os
import struct

import numpy as np
import pytest

from tests.ema_ref import merged, ref_ema_decay_at, ref_ema_update
from tests.optim_ref import decay_ranges_of, moving_stat_mask
from tests.test_gpu_optimizer import LR, NETS, bits, make_net, net_inputs, same, step_kernels

pytestmark = pytest.mark.gpu

STEP_FAMILIES = ("sgd_", "sgdm_", "adam_", "lamb_", "lars_", "seg_", "clip_")
SGDM = dict(momentum=0.9, weight_decay=5e-4, nesterov=True, decay_bias_and_norm=True)
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, decoupled=True)
LR_OF = {"plain": LR, "sgdm": LR, "adamw": 1e-3}  # (rates at which four steps of each kind keep the loss finite)


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def arm(net, kind):
    if kind == "sgdm":
        net.set_optimizer(**SGDM)
    elif kind == "adamw":
        net.set_adam(**ADAMW)


def state_of(net, kind):
    if kind == "sgdm":
        return [net.get_velocity()]
    if kind == "adamw":
        m, v, t = net.get_adam_state()
        return [m, v, np.asarray([t], np.float32)]
    return []


def averaged_ranges(layout, average_stats=False):
    """the container's table, from the layout: everything but BatchNorm2D's moving statistics, neighbours merged"""
    n = sum(e["params"] for e in layout)
    return [(0, n)] if average_stats else merged(decay_ranges_of(layout, bias_and_norm=True))


def follow(net, shadow, ranges, t, tag):
    """after one optimizer step: the shadow on the device is the restatement's update of the previous shadow -> the new shadow"""
    p = net.get_params()
    want = ref_ema_update(shadow, p, ref_ema_decay_at(0.9, True, t), ranges)
    got = net.get_ema()
    print(f"{tag}: update {t + 1}, decay {ref_ema_decay_at(0.9, True, t)!r}, shadow differs at {int((bits(got) != bits(want)).sum())} of {p.size}")
    assert same(got, want), tag + ": shadow"
    assert net.ema_updates() == t + 1, tag
    return want


# ---- 1. the shadow follows the arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,kind", [("small_bn", "plain"), ("small_bn", "sgdm"), ("small_bn", "adamw"), ("alexnet", "plain"),
                                        ("alexnet", "sgdm"), ("alexnet", "adamw")])
def test_shadow_follows_the_restatement(T, which, kind):
    """set_ema(0.9, warmup) then four train_steps: the shadow starts as the parameters' words and is ref_ema_update of itself after
    every step, bit for bit; BatchNorm2D's moving statistics are the model's words unless average_stats; the counter reads 1..4"""
    layout, p0, x, labels = net_inputs(T, which, 700)
    moving = moving_stat_mask(layout)
    assert moving.any() == (which == "small_bn")
    for average_stats in ((False, True) if moving.any() else (False,)):
        ranges = averaged_ranges(layout, average_stats)
        net = make_net(which)
        net.set_params(p0)
        arm(net, kind)
        with pytest.raises(Exception, match="get_ema"):
            net.get_ema()
        net.set_ema(0.9, warmup=True, average_stats=average_stats)
        shadow = net.get_ema()
        assert same(shadow, net.get_params()) and same(shadow, p0) and net.ema_updates() == 0
        for t in range(4):
            net.train_step(x, labels, LR_OF[kind])
            assert np.isfinite(net.last_loss())
            shadow = follow(net, shadow, ranges, t, f"{which} {kind} stats={average_stats}")
            p = net.get_params()
            if moving.any() and not average_stats:
                assert same(shadow[moving], p[moving]), "the moving statistics follow the model"
            if moving.any() and average_stats:
                assert not same(shadow[moving], p[moving]), "the moving statistics are averaged too"
            assert not same(shadow[~moving], p[~moving])
        net.close()


# ---- 2. the average moves no parameter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,kind", [("small_bn", "sgdm"), ("alexnet", "plain"), ("alexnet", "adamw")])
def test_ema_moves_no_parameter(T, which, kind):
    """the same net and inputs with the average on and with set_ema never called: parameters, gradients, optimizer state and losses
    agree bit for bit after every one of four steps, and every layer's get_output() is the other net's"""
    from cnn_amd import hostapi

    spec, in_shape, B = NETS[which]
    layout, p0, x, labels = net_inputs(T, which, 710)
    names = hostapi._layer_names(spec)
    a, b = make_net(which), make_net(which)
    for net in (a, b):
        net.set_params(p0)
        arm(net, kind)
    a.set_ema(0.9, warmup=True)
    for step in range(4):
        a.train_step(x, labels, LR_OF[kind])
        b.train_step(x, labels, LR_OF[kind])
        assert a.last_loss() == b.last_loss() and np.isfinite(a.last_loss()), step
        assert same(a.get_params(), b.get_params()), f"step {step}: parameters"
        assert same(a.get_grads(), b.get_grads()), f"step {step}: gradients"
        assert all(same(u, v) for u, v in zip(state_of(a, kind), state_of(b, kind))), f"step {step}: optimizer state"
    for name, e in zip(names, layout):
        shape = (B,) + tuple(e["out"])
        assert same(a.layer_output(name, shape), b.layer_output(name, shape)), name
    a.close()
    b.close()


# ---- 3. launches -------------------------------------------------------------------------------------------------------------------------
def call_kernels(T, net, x, labels):
    from cnn_amd import capi

    T.cuda.synchronize()
    capi.kernel_timing(1)
    net.train_step(x, labels, 1e-3)
    net.flush()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    return {k: cnt for k, (cnt, _) in rep.items()}


def family(kernels, prefixes):
    return {k.split("|")[0]: cnt for k, cnt in kernels.items() if k.startswith(prefixes)}


@pytest.mark.parametrize("which,kind", [("small_bn", "plain"), ("small_bn", "adamw"), ("alexnet", "plain"), ("alexnet", "sgdm")])
def test_one_ema_launch_per_step(T, which, kind, lib_option):
    """per train_step exactly one ema_ launch and no aswap_ launch; the step families launch what a net without the average launches
    in the plain sequence (the fused step tail declines while the average is on: the twin runs with NO_FUSED_TAIL); after set_ema(0)
    no ema_ launch"""
    layout, p0, x, labels = net_inputs(T, which, 720)
    a, b = make_net(which), make_net(which)
    for net in (a, b):
        net.set_params(p0)
        arm(net, kind)
    a.set_ema(0.999)
    for step in range(3):
        ka = call_kernels(T, a, x, labels)
        lib_option("NO_FUSED_TAIL", "1")
        kb = call_kernels(T, b, x, labels)
        lib_option("NO_FUSED_TAIL", None)
        assert family(ka, ("ema_",)) == {"ema_vec": 1}, (step, family(ka, ("ema_",)))
        assert not family(ka, ("aswap_",)) and not family(kb, ("ema_", "aswap_"))
        assert family(ka, STEP_FAMILIES) == family(kb, STEP_FAMILIES) and family(ka, STEP_FAMILIES), (step, family(ka, STEP_FAMILIES))
        assert {k: c for k, c in ka.items() if not k.startswith("ema_")} == kb, step
    assert same(a.get_params(), b.get_params())
    a.set_ema(0)
    assert a.ema_updates() == 3 and a.get_ema() is not None
    ka = call_kernels(T, a, x, labels)
    assert not family(ka, ("ema_", "aswap_")) and a.ema_updates() == 3
    a.close()
    b.close()


def test_ema_off_is_the_default_path(T, golden_dir):
    """after set_ema(0.9) and set_ema(0) three train_steps of a fresh reference net launch exactly the committed golden list (the
    comparison of test_default_path_is_untouched) and end with the never-armed net's parameters"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 340)
    golden = json.load(open(os.path.join(golden_dir, "train_step_kernels_before_optimizer.json")))
    runs = {}
    for mode in ("never", "off_again"):
        net = make_net("alexnet")
        net.set_params(p0)
        if mode == "off_again":
            net.set_ema(0.9)
            net.set_ema(0)
        runs[mode] = (step_kernels(T, net, x, labels), net.get_params())
        net.close()
    assert runs["off_again"][0] == golden, sorted(set(runs["off_again"][0].items()) ^ set(golden.items()))
    assert runs["never"][0] == golden and same(runs["never"][1], runs["off_again"][1])


@pytest.mark.parametrize("clip", [False, True])
def test_one_update_per_accumulation_window(T, clip):
    """set_grad_accumulation(3) [and set_grad_clip]: one ema_ launch in the closing call only, the counter advances once per window,
    the shadow is the restatement's bit for bit"""
    which = "small_bn"
    layout, p0, x, labels = net_inputs(T, which, 730)
    ranges = averaged_ranges(layout)
    net = make_net(which)
    net.set_params(p0)
    arm(net, "adamw")
    if clip:
        net.set_grad_clip(1e-3)
    net.set_grad_accumulation(3)
    net.set_ema(0.9, warmup=True)
    shadow = net.get_ema()
    for w in range(2):
        for j in range(3):
            k = call_kernels(T, net, x, labels)
            tag = f"clip={clip} window {w} call {j + 1}"
            if j < 2:
                assert not family(k, ("ema_", "aswap_")) and net.ema_updates() == w, tag
                assert same(net.get_ema(), shadow), tag
            else:
                assert family(k, ("ema_",)) == {"ema_vec": 1} and not family(k, ("aswap_",)), tag
                assert bool(family(k, ("clip_",))) == clip
                shadow = follow(net, shadow, ranges, w, tag)
    net.close()


# ---- 4. swap -----------------------------------------------------------------------------------------------------------------------------
def eval_logits(net, x_host):
    from cnn_amd import hostapi

    hostapi.load().cnnh_set_no_grad(1)
    try:
        return net.forward_host(x_host)
    finally:
        hostapi.load().cnnh_set_no_grad(0)


@pytest.mark.parametrize("which", ["small_bn", "alexnet"])
def test_swap_for_evaluation_and_export(T, which, tmp_path):
    from cnn_amd import capi

    layout, p0, x, labels = net_inputs(T, which, 740)
    x_host = x.cpu().numpy()
    net, twin = make_net(which), make_net(which)
    net.swap_ema()  # before any set_ema: nothing
    T.cuda.synchronize()
    capi.kernel_timing(1)
    net.swap_ema()
    assert capi.kernel_timing_report() == {} and not net.ema_swapped()
    capi.kernel_timing(0)
    for n_ in (net, twin):
        n_.set_params(p0)
        arm(n_, "sgdm")
        n_.set_ema(0.9, warmup=True)
        for _ in range(3):
            n_.train_step(x, labels, LR)
    params, shadow = net.get_params(), net.get_ema()
    assert not same(params, shadow)
    T.cuda.synchronize()
    capi.kernel_timing(1)
    net.swap_ema()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    assert [(k.split("|")[0], cnt) for k, (cnt, _) in rep.items()] == [("aswap_vec", 1)], rep
    assert net.ema_swapped() and same(net.get_params(), shadow) and same(net.get_ema(), params)
    # evaluation: the logits of a fresh net that was given the shadow
    fresh = make_net(which)
    fresh.set_params(shadow)
    want = eval_logits(fresh, x_host)
    fresh.close()
    got = eval_logits(net, x_host)
    assert same(got, want) and np.isfinite(got).all()
    assert same(net.get_params(), shadow), "an eval-mode forward pass leaves the arena alone"
    # export: the reference's .model format holds the average
    out = tmp_path / "averaged.model"
    net.save_checkpoint(out)
    assert same(np.fromfile(out, dtype=np.float32), shadow)
    net.swap_ema()
    assert not net.ema_swapped() and same(net.get_params(), params) and same(net.get_ema(), shadow)
    # a step taken while swapped swaps back first
    net.swap_ema()
    k = call_kernels(T, net, x, labels)
    twin.train_step(x, labels, 1e-3)
    assert family(k, ("aswap_",)) == {"aswap_vec": 1} and family(k, ("ema_",)) == {"ema_vec": 1}, k
    assert not net.ema_swapped()
    assert same(net.get_params(), twin.get_params()) and same(net.get_ema(), twin.get_ema()) and net.ema_updates() == twin.ema_updates() == 4
    # the context manager restores on exit, also when the body raises
    params, shadow = net.get_params(), net.get_ema()
    with net.averaged() as inside:
        assert inside is net and net.ema_swapped() and same(net.get_params(), shadow)
    assert not net.ema_swapped() and same(net.get_params(), params) and same(net.get_ema(), shadow)
    with pytest.raises(ZeroDivisionError):
        with net.averaged():
            assert net.ema_swapped()
            1 / 0
    assert not net.ema_swapped() and same(net.get_params(), params) and same(net.get_ema(), shadow)
    # update_gradients swaps back as well
    net.swap_ema()
    net.update(1e-3)
    assert not net.ema_swapped() and net.ema_updates() == 5
    net.close()
    twin.close()


# ---- 5. state file -----------------------------------------------------------------------------------------------------------------------
def test_state_file_round_trip_and_status_codes(T, tmp_path):
    from cnn_amd import capi

    which = "small_bn"
    layout, p0, x, labels = net_inputs(T, which, 750)
    a = make_net(which)
    a.set_params(p0)
    arm(a, "adamw")
    none_yet = str(tmp_path / "none.emastate")
    assert a.lib.cnnh_net_save_ema_state(a.h, none_yet.encode()) == 4 and not os.path.exists(none_yet)
    opt_before = str(tmp_path / "before.optstate")
    a.save_optimizer_state(opt_before)
    a.set_ema(0.9, warmup=True, average_stats=True)
    opt_with = str(tmp_path / "with.optstate")
    a.save_optimizer_state(opt_with)
    assert open(opt_before, "rb").read() == open(opt_with, "rb").read(), "the optimizer state file does not know about the average"
    for _ in range(3):
        a.train_step(x, labels, LR_OF["adamw"])
    model, opt, state = str(tmp_path / "s3.model"), str(tmp_path / "s3.optstate"), str(tmp_path / "s3.emastate")
    a.save_checkpoint(model)
    a.save_optimizer_state(opt)
    a.save_ema_state(state)
    raw = open(state, "rb").read()
    assert len(raw) == 40 + 4 * a.n_params and raw[:8] == b"CNNAEMA1"
    assert struct.unpack("<QQfIII", raw[8:40]) == (a.n_params, 3, float(np.float32(0.9)), 1, 1, 0)
    assert same(np.frombuffer(raw[40:], np.float32), a.get_ema())
    for _ in range(2):
        a.train_step(x, labels, LR_OF["adamw"])
    b = make_net(which)
    b.load_checkpoint(model)
    b.load_optimizer_state(opt)
    # failures first: nothing changes
    b.set_ema(0.5)
    b.train_step(x, labels, LR_OF["adamw"])
    b.load_checkpoint(model)
    b.load_optimizer_state(opt)
    held = (b.get_ema(), b.ema_updates())
    short, header_only, bad_decay, other_file = (str(tmp_path / n) for n in ("short", "header", "decay", "other"))
    open(short, "wb").write(raw[:-8])
    open(header_only, "wb").write(raw[:40])
    open(bad_decay, "wb").write(raw[:24] + struct.pack("<f", 1.5) + raw[28:])
    other = make_net("alexnet")
    other.set_ema(0.9)
    other.save_ema_state(other_file)
    load = lambda path: b.lib.cnnh_net_load_ema_state(b.h, path.encode())
    assert load(str(tmp_path / "missing")) == 1
    assert load(short) == 2 and load(header_only) == 2 and load(bad_decay) == 2 and load(opt) == 2
    assert load(other_file) == 3
    assert other.lib.cnnh_net_load_ema_state(other.h, state.encode()) == 3
    other.close()
    with pytest.raises(FileNotFoundError):
        b.load_ema_state(str(tmp_path / "missing"))
    with pytest.raises(capi.CnnAmdError, match="n_params"):
        b.load_ema_state(other_file)
    assert same(b.get_ema(), held[0]) and b.ema_updates() == held[1] == 1
    k = call_kernels(T, b, x, labels)  # (the options are unchanged too: decay 0.5, no warm-up, the moving statistics copied)
    want = ref_ema_update(held[0], b.get_params(), 0.5, averaged_ranges(layout))
    assert same(b.get_ema(), want) and family(k, ("ema_",)) == {"ema_vec": 1}
    # the round trip
    b.load_checkpoint(model)
    b.load_optimizer_state(opt)
    b.load_ema_state(state)
    assert b.ema_updates() == 3
    for _ in range(2):
        b.train_step(x, labels, LR_OF["adamw"])
    assert same(b.get_params(), a.get_params()), "(the two nets took the same steps)"
    assert same(b.get_ema(), a.get_ema()) and b.ema_updates() == a.ema_updates() == 5
    a.close()
    b.close()


# ---- 6. forced one-rank exchange ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["alexnet", "small_bn"])
def test_forced_one_rank_exchange(T, which, lib_option):
    """DP_FORCE_EXCHANGE with ONE rank (every sum is an identity): shadow, parameters and counter of four steps equal the
    no-communicator run's"""
    from cnn_amd.dp import RcclComm

    layout, p0, x, labels = net_inputs(T, which, 760)
    comm = RcclComm(None, 1, 0)
    outs = []
    for use_comm in (False, True):
        net = make_net(which)
        net.set_params(p0)
        arm(net, "sgdm")
        net.set_ema(0.9, warmup=True)
        if use_comm:
            net.set_comm(comm.handle, 1)
            lib_option("DP_FORCE_EXCHANGE", "1")
        for _ in range(4):
            net.train_step(x, labels, LR)
        outs.append((net.get_params(), net.get_ema(), net.ema_updates()))
        net.close()
        lib_option("DP_FORCE_EXCHANGE", None)
    comm.destroy()
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2] == 4


# ---- 7. reset_ema after load_checkpoint ------------------------------------------------------------------------------------------------
def test_reset_after_load_checkpoint(T, tmp_path):
    which = "small_bn"
    layout, p0, x, labels = net_inputs(T, which, 770)
    net = make_net(which)
    net.set_params(p0)
    net.reset_ema()  # (before any set_ema: nothing)
    net.set_ema(0.9)
    model = str(tmp_path / "start.model")
    net.save_checkpoint(model)
    for _ in range(2):
        net.train_step(x, labels, LR)
    assert net.ema_updates() == 2 and not same(net.get_ema(), p0)
    net.load_checkpoint(model)
    net.reset_ema()
    assert same(net.get_params(), p0) and same(net.get_ema(), p0) and net.ema_updates() == 0
    net.close()
