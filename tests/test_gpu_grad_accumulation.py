"""Gradient accumulation over micro-batches in the container (Sequential::set_grad_accumulation) on the device, through cnn_amd.hostapi.
A window of k container steps is ONE optimizer step on the summed gradients: the reference is a second net that runs the plain sequence
per micro-batch, NumPy sums its gradient arenas in float32 (a copy, then adds) and takes the kind's reference step with grad_scale 1/k.
Every comparison of parameters, state and accumulator is bit-exact; the one tolerance check (the window IS the large batch) is held to
the project's REL_TOL against the oracle."""
import json
import os

import numpy as np
import pytest

from cnn_amd import stacks as S
from tests.adam_ref import ref_adam_step, ref_clip, ref_total_norm
from tests.lamb_ref import ref_lamb_step, ref_lars_step, ref_segment_norms, segment_table_of
from tests.optim_ref import decay_ranges_of, moving_stat_mask, ref_sgd_step
from tests.test_gpu_optimizer import LR, NETS, SMALL_BN, bits, make_net, net_inputs, same, step_kernels
from tests.util import REL_TOL, assert_close, assert_close_arbitrated, he_init, uniform01

SMALL_PLAIN = [item for item in SMALL_BN if item[0] != "bn"]  # small_bn without its BatchNorm layers
PLAIN_SHAPE = (3, 32, 32)
K = 3
THIRD = float(np.float32(1) / np.float32(3))
STEP_FAMILIES = ("sgd_", "sgdm_", "adam_", "lamb_", "lars_", "seg_", "clip_")


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def micro_batches(T, which, seed, count):
    """`count` different micro-batches of the net's batch size: (x, labels) on the device"""
    spec, in_shape, B = NETS[which]
    return [(T.from_numpy(uniform01(seed + 10 * i, (B,) + in_shape)).cuda(), T.from_numpy(((np.arange(B) + i) % 3).astype(np.int32)).cuda())
            for i in range(count)]


def accumulate(acc, g):
    """the accumulator's arithmetic on the host: a copy, then float32 adds"""
    if acc is None:
        return g.copy()
    out = acc + g
    assert out.dtype == np.float32
    return out


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.uint32).astype(np.int64) - b.view(np.uint32).astype(np.int64))  # (non-negative finite values)


# ---- the optimizer kinds: how net A is armed, which state arenas it has, the reference step on (p, acc, state) with grad_scale 1/k --------
SGDM = dict(momentum=0.9, weight_decay=5e-4, nesterov=True, decay_bias_and_norm=True)
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, decoupled=True)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-4, decoupled=False)
LAMB = dict(weight_decay=1e-2)
LARS = dict(momentum=0.9, weight_decay=5e-4)


class Kind:
    def __init__(self, name, layout):
        self.name, self.layout = name, layout
        self.n_state = {"plain": 0, "sgdm": 1, "adamw": 2, "adam": 2, "lamb": 2, "lars": 1}[name]
        self.counts_steps = name in ("adamw", "adam", "lamb")
        if name in ("lamb", "lars"):
            self.bounds, self.flags = segment_table_of(layout)

    def arm(self, net):
        if self.name == "sgdm":
            net.set_optimizer(**SGDM)
        elif self.name in ("adamw", "adam"):
            net.set_adam(**(ADAMW if self.name == "adamw" else ADAM))
        elif self.name == "lamb":
            net.set_lamb(**LAMB)
        elif self.name == "lars":
            net.set_lars(**LARS)

    def state_of(self, net):
        if self.name in ("sgdm", "lars"):
            return [net.get_velocity()], None
        if self.n_state == 2:
            m, v, t = net.get_adam_state()
            return [m, v], t
        return [], None

    def step(self, net_a, p, g, state, t, grad_scale, tag):
        """-> (p', state'); t: the 1-based number of this optimizer step.  LAMB / LARS take net A's device norms of this step
        (trust_stats), held to the fp64 norms within one ulp, and its ratios must be the reference's bit for bit"""
        if self.name == "plain":
            return ref_sgd_step(p, g, None, LR, grad_scale=grad_scale)[0], []
        if self.name == "sgdm":
            p_new, v = ref_sgd_step(p, g, state[0], LR, SGDM["momentum"], SGDM["weight_decay"], SGDM["nesterov"], grad_scale,
                                    decay_ranges_of(self.layout, SGDM["decay_bias_and_norm"]))
            return p_new, [v]
        if self.name in ("adamw", "adam"):
            kw = ADAMW if self.name == "adamw" else ADAM
            p_new, m, v = ref_adam_step(p, g, state[0], state[1], t, LR, grad_scale=grad_scale, decay_ranges=decay_ranges_of(self.layout, False), **kw)
            return p_new, [m, v]
        wn, un, ratio = net_a.trust_stats()
        assert np.all(ulps(wn, ref_segment_norms(p, self.bounds)) <= 1), tag + " w_norm"
        if self.name == "lamb":
            p_new, m, v, r, want_ratio = ref_lamb_step(p, g, state[0], state[1], self.bounds, self.flags, t, LR, wn, un, eps=1e-6,
                                                       weight_decay=LAMB["weight_decay"], grad_scale=grad_scale)
            assert np.all(ulps(un, ref_segment_norms(r, self.bounds)) <= 1), tag + " u_norm"
            assert same(ratio, want_ratio), tag + " ratio"
            return p_new, [m, v]
        # (the device reports (float)norm * grad_scale: the fp64 norm or one of its fp32 neighbours, times the scale in fp32)
        norm = ref_segment_norms(g, self.bounds)
        near = [np.nextafter(norm, np.float32(np.inf)), norm, np.maximum(np.nextafter(norm, np.float32(-np.inf)), np.float32(0))]
        assert np.all(np.any([bits(c * np.float32(grad_scale)) == bits(un) for c in near], axis=0)), tag + " g_norm"
        p_new, v, _, want_ratio = ref_lars_step(p, g, state[0], self.bounds, self.flags, LR, wn, un, LARS["momentum"], LARS["weight_decay"],
                                                grad_scale=grad_scale, norm_is_scaled=True)
        assert same(ratio, want_ratio), tag + " ratio"
        return p_new, [v]


def run_windows(T, which, kind_name, windows, seed):
    """net A: K train_steps per window under set_grad_accumulation(K); net B: the plain sequence per micro-batch, the sum and the step
    on the host.  Checks every call."""
    layout, p0, _, _ = net_inputs(T, which, seed)
    moving = moving_stat_mask(layout)
    kind = Kind(kind_name, layout)
    batches = micro_batches(T, which, seed + 1, K * windows)
    a, b = make_net(which), make_net(which)
    a.set_params(p0)
    b.set_params(p0)
    with pytest.raises(Exception, match="get_accumulated_grads"):
        a.get_accumulated_grads()  # (accumulation was never on)
    kind.arm(a)
    a.set_grad_accumulation(K)
    assert a.accumulation_phase() == 0 and not np.any(a.get_accumulated_grads())
    state, t0 = kind.state_of(a)
    for w in range(windows):
        p_start, acc = a.get_params(), None
        for j in range(K):
            x, labels = batches[w * K + j]
            b.forward_backward(x, labels)
            loss, g, p_b = b.last_loss(), b.get_grads(), b.get_params()  # (p_b: B's forward pass moved the moving statistics)
            acc = accumulate(acc, g)
            a.train_step(x, labels, LR)
            tag = f"{which} {kind_name} window {w} call {j + 1}"
            assert a.last_loss() == loss, tag
            assert a.accumulation_phase() == (j + 1) % K, tag
            got_p = a.get_params()
            got_state, got_t = kind.state_of(a)
            if j < K - 1:
                assert same(a.get_accumulated_grads(), acc), tag + ": accumulator"
                assert same(got_p, p_b), tag + ": a parameter moved inside the window"
                assert same(got_p[~moving], p_start[~moving]), tag + ": more than the moving statistics differs from the window's start"
                assert moving.any() == (not same(got_p, p_start)), tag
                assert all(same(x_, y_) for x_, y_ in zip(got_state, state)), tag + ": optimizer state moved inside the window"
                assert got_t == (None if t0 is None else t0 + w), tag
                continue
            assert same(a.get_accumulated_grads(), acc), tag + ": accumulator"
            p_new, state = kind.step(a, p_b, acc, state, None if t0 is None else t0 + w + 1, THIRD, tag)
            print(f"{tag}: loss {loss!r}, parameters differ at {int((bits(got_p) != bits(p_new)).sum())} of {p_new.size}")
            assert same(got_p, p_new), tag + ": parameters"
            assert all(same(x_, y_) for x_, y_ in zip(got_state, state)), tag + ": state"
            assert got_t == (None if t0 is None else t0 + w + 1), tag + ": ONE optimizer step per window"
            assert same(p_new[moving], p_b[moving]) and not same(p_new, p_b)
            b.set_params(p_new)
    a.close()
    b.close()


# ---- 1. bit-exact windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,kind", [("small_bn", "plain"), ("small_bn", "sgdm"), ("small_bn", "adamw"), ("small_bn", "lamb"), ("small_bn", "lars"),
                                        ("alexnet", "plain"), ("alexnet", "adam")])
def test_windows_equal_the_host_accumulated_step(T, which, kind):
    """k = 3, two windows, a different micro-batch in every call.  After every call parameters and every state arena agree with the
    host-stepped net bit for bit and get_accumulated_grads() is NumPy's sum; in calls 1 and 2 only BatchNorm2D's moving statistics
    differ from the window's start; the Adam / LAMB step counter is +1 per window; accumulation_phase() reads 1, 2, 0"""
    run_windows(T, which, kind, 2, 600)


# ---- 2. clipping ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_clip_reads_the_accumulator(T):
    """small_bn, momentum SGD, max_norm = half of the first window's norm: last_grad_norm() is ref_total_norm / ref_clip on the
    accumulated gradient with scale 1/3, the step runs on the clipped accumulator, parameters and velocity bit for bit"""
    which = "small_bn"
    layout, p0, _, _ = net_inputs(T, which, 610)
    kind = Kind("sgdm", layout)
    batches = micro_batches(T, which, 611, 2 * K)
    a, b = make_net(which), make_net(which)
    a.set_params(p0)
    b.set_params(p0)
    kind.arm(a)
    a.set_grad_accumulation(K)
    state, max_norm = [np.zeros(p0.size, np.float32)], None
    for w in range(2):
        acc = None
        for j in range(K):
            x, labels = batches[w * K + j]
            b.forward_backward(x, labels)
            acc = accumulate(acc, b.get_grads())
            if max_norm is None and j == K - 1:
                max_norm = 0.5 * float(ref_total_norm(acc, THIRD))
                a.set_grad_clip(max_norm)  # (set_grad_clip leaves the open window alone)
                assert a.accumulation_phase() == K - 1
            a.train_step(x, labels, LR)
        total = ref_total_norm(acc, THIRD)
        norm, coef = a.last_grad_norm()
        clipped, want_coef = ref_clip(acc, total, max_norm)  # (grad_scale is folded into `total` already)
        print(f"window {w}: device norm {norm!r}, reference {total!r}, coefficient {coef!r} / {want_coef!r}")
        assert bits(np.asarray([norm]))[0] == bits(np.asarray([total]))[0], w
        assert bits(np.asarray([coef]))[0] == bits(np.asarray([want_coef]))[0] and (w > 0 or coef < 1), w
        assert same(a.get_accumulated_grads(), clipped), "the clip scales the accumulator in place"
        p_new, state = kind.step(a, b.get_params(), clipped, state, None, THIRD, f"clip window {w}")
        assert same(a.get_params(), p_new) and same(a.get_velocity(), state[0]), w
        b.set_params(p_new)
    a.close()
    b.close()


# ---- 3. launch log -------------------------------------------------------------------------------------------------------------------------
def call_kernels(T, net, x, labels):
    from cnn_amd import capi

    T.cuda.synchronize()
    capi.kernel_timing(1)
    net.train_step(x, labels, 1e-3)
    net.flush()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    return {k: cnt for k, (cnt, _) in rep.items()}


def family_launches(kernels, prefixes):
    return sum(cnt for k, cnt in kernels.items() if k.startswith(prefixes))


@pytest.mark.gpu
@pytest.mark.parametrize("arm,expect", [("plain", ("sgd_",)), ("sgdm", ("sgdm_",)), ("adam_clip", ("adam_", "clip_")), ("lamb", ("lamb_", "seg_")),
                                        ("lars", ("lars_", "seg_"))])
def test_one_accumulate_launch_per_call_and_the_step_in_the_closing_call_only(T, arm, expect):
    """k = 3 on the reference net: every call launches exactly one gacc_ kernel (the first opens the window, the others add); the step
    families appear in the closing call only, and there the active kind's do"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 620)
    net = make_net("alexnet")
    net.set_params(p0)
    if arm == "adam_clip":
        net.set_adam(**ADAM)
        net.set_grad_clip(1e-3)
    else:
        Kind(arm, layout).arm(net)
    net.set_grad_accumulation(K)
    for w in range(2):
        for j in range(K):
            kernels = call_kernels(T, net, x, labels)
            gacc = {k.split("|")[0]: cnt for k, cnt in kernels.items() if k.startswith("gacc_")}
            assert gacc == {"gacc_vec_first" if j == 0 else "gacc_vec_add": 1}, (w, j, gacc)
            steps = {k: cnt for k, cnt in kernels.items() if k.startswith(STEP_FAMILIES)}
            if j < K - 1:
                assert not steps, (w, j, steps)
            else:
                assert all(family_launches(kernels, (fam,)) >= 1 for fam in expect), (w, j, steps)
                assert family_launches(kernels, STEP_FAMILIES) == family_launches(kernels, expect), (w, j, steps)
    net.close()


@pytest.mark.gpu
def test_k_1_is_the_default_path(T, golden_dir):
    """after set_grad_accumulation(3) and back to 1, three train_steps of a fresh reference net launch exactly the committed golden list
    (the comparison of test_default_path_is_untouched), no gacc_ kernel among them, and end with the never-armed net's parameters; a
    net that ran a whole window and returned to 1 launches no gacc_ kernel either and steps like a net that never accumulated"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 340)
    golden = json.load(open(os.path.join(golden_dir, "train_step_kernels_before_optimizer.json")))
    assert not any(k.startswith("gacc_") for k in golden)
    runs = {}
    for mode in ("never", "off_again"):
        net = make_net("alexnet")
        net.set_params(p0)
        if mode == "off_again":
            net.set_grad_accumulation(K)
            net.set_grad_accumulation(1)
        runs[mode] = (step_kernels(T, net, x, labels), net.get_params())
        net.close()
    assert runs["off_again"][0] == golden, sorted(set(runs["off_again"][0].items()) ^ set(golden.items()))
    assert runs["never"][0] == golden and same(runs["never"][1], runs["off_again"][1])
    used = make_net("alexnet")
    used.set_params(p0)
    used.set_grad_accumulation(K)
    for _ in range(K):
        used.train_step(x, labels, 1e-3)
    assert used.accumulation_phase() == 0
    used.set_grad_accumulation(1)
    fresh = make_net("alexnet")
    fresh.set_params(used.get_params())
    after = step_kernels(T, used, x, labels)
    for _ in range(3):
        fresh.train_step(x, labels, 1e-3)
    assert not any(k.startswith("gacc_") for k in after), after
    assert same(used.get_params(), fresh.get_params())
    used.close()
    fresh.close()


# ---- 4. the window IS the large batch ------------------------------------------------------------------------------------------------------
BIG_B, MICRO_B = 8, 2


def plain_case():
    from oracle import pyoracle as O

    layout = S.walk(SMALL_PLAIN, *PLAIN_SHAPE)
    p0 = he_init(layout, 630)
    x = uniform01(631, (BIG_B,) + PLAIN_SHAPE)
    labels = (np.arange(BIG_B) % 3).astype(np.int32)
    bounds, _ = segment_table_of(layout)
    names = []
    for e in layout:
        if e["params"]:
            names += [f"{e['kind']}{len(names) // 2 + 1}.w", f"{e['kind']}{len(names) // 2 + 1}.b"]
    return O, layout, p0, x, labels, [(n, int(lo), int(hi)) for n, lo, hi in zip(names, bounds[:-1], bounds[1:])]


def oracle_grads(O, p0, x, labels, f64=False, masks_from=None):
    net = O.SeqNet(SMALL_PLAIN, PLAIN_SHAPE, f64=f64)
    net.params[:] = p0
    logits = net.forward(x)
    _, delta = O.cross_entropy_backward(O.softmax(logits, f64=f64), labels, f64=f64)
    net.backward(delta, masks_from=masks_from)
    return net.grads.copy(), net


def test_oracle_micro_batch_sums_meet_the_bar_against_its_own_full_batch():
    """(CPU) the chosen inputs do not eat the tolerance by themselves: the oracle's own gradients of four micro-batches of 2, summed in
    float32 and scaled by 0.25, against its full-batch gradient at B = 8 -- per parameter tensor at REL_TOL, margins recorded"""
    O, layout, p0, x, labels, tensors = plain_case()
    full, _ = oracle_grads(O, p0, x, labels)
    acc = None
    for i in range(0, BIG_B, MICRO_B):
        acc = accumulate(acc, oracle_grads(O, p0, x[i:i + MICRO_B], labels[i:i + MICRO_B])[0])
    mean = acc * np.float32(0.25)
    assert len(tensors) == 6 and tensors[-1][2] == full.size
    worst = max(assert_close(mean[lo:hi], full[lo:hi], REL_TOL, f"oracle micro-batch sums, grad {name}") for name, lo, hi in tensors)
    print(f"oracle micro-batch sums against its own full batch: worst tensor-normalised error {worst:.3e}")
    assert worst <= 0.1 * REL_TOL, "the inputs alone use more than a tenth of the tolerance"


@pytest.mark.gpu
def test_a_window_is_the_large_batch(T):
    """small_plain has no BatchNorm, so in real arithmetic the mean of four micro-batch gradients IS the gradient of the batch of 8:
    get_accumulated_grads() * 0.25 after a k = 4 window of micro-batches of 2 against the oracle's full-batch gradient at B = 8, per
    parameter tensor at REL_TOL, fp64-arbitrated.  The oracle takes its ReLU / MaxPool decisions from the device's forward tensors
    (SeqNet.backward's masks_from, as the stack parity tests do): both sides differentiate the same piecewise-linear function"""
    from cnn_amd import hostapi

    O, layout, p0, x, labels, tensors = plain_case()
    names = hostapi._layer_names(SMALL_PLAIN)
    net = hostapi.HostSequential(SMALL_PLAIN, PLAIN_SHAPE)
    net.set_params(p0)
    net.set_grad_accumulation(BIG_B // MICRO_B)
    xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    relu_out = {idx: [] for idx, e in enumerate(layout) if e["kind"] == "relu"}
    for i in range(0, BIG_B, MICRO_B):
        net.train_step(xd[i:i + MICRO_B], ld[i:i + MICRO_B], 0.0)  # (lr 0: the closing call's step leaves the parameters)
        for idx in relu_out:
            relu_out[idx].append(net.layer_output(names[idx], (MICRO_B,) + layout[idx]["out"]))
    assert net.accumulation_phase() == 0 and same(net.get_params(), p0)
    got = net.get_accumulated_grads() * np.float32(0.25)
    net.close()
    masks_from = {}
    for idx, parts in relu_out.items():
        masks_from[idx] = np.concatenate(parts)
        if layout[idx + 1]["kind"] == "pool":
            masks_from[idx + 1] = masks_from[idx]  # the pool's input IS this ReLU's output
    g32, o32 = oracle_grads(O, p0, x, labels, masks_from=masks_from)
    g64, _ = oracle_grads(O, p0, x, labels, f64=True, masks_from=masks_from)
    flipped = sum(int(np.count_nonzero((masks_from[idx] <= 0) != (o32.acts[idx] <= 0))) for idx in relu_out)
    assert flipped <= 2, flipped
    for name, lo, hi in tensors:
        e = assert_close_arbitrated(got[lo:hi], g32[lo:hi], g64[lo:hi], REL_TOL, 2.0, f"k=4 window vs B=8 oracle, grad {name}")
        print(f"grad {name}: tensor-normalised error {e:.3e} against the fp32 oracle's full batch")


# ---- 5. one-rank exchange ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["DP_FORCE_EXCHANGE", "DP_FORCE_BUCKETS"])
def test_forced_one_rank_exchange_of_the_accumulator(T, switch, lib_option):
    """a one-rank communicator with the exchange forced on (every sum is an identity): a k = 3 window on small_bn under Adam -- ONE
    all-reduce over the accumulator in the closing call, none inside backward(), allreduce_gradients() a no-op -- ends bit-identical
    to the same window without a communicator"""
    from cnn_amd import capi
    from cnn_amd.dp import RcclComm

    if capi.load().cnn_comm_available() == 0:
        pytest.skip("the library was built without RCCL")
    which = "small_bn"
    layout, p0, _, _ = net_inputs(T, which, 640)
    batches = micro_batches(T, which, 641, K)
    comm = RcclComm(None, 1, 0)
    outs = []
    for use_comm in (False, True):
        net = make_net(which)
        net.set_params(p0)
        net.set_adam(**ADAM)
        net.set_grad_accumulation(K)
        if use_comm:
            net.set_comm(comm.handle, 1)
            lib_option(switch, "1")
        losses = []
        for x, labels in batches:
            net.train_step(x, labels, LR)
            net.allreduce_gradients()
            losses.append(net.last_loss())
        outs.append((losses, net.get_params(), net.get_accumulated_grads()) + net.get_adam_state())
        net.close()
        lib_option(switch, None)
    comm.destroy()
    assert outs[0][0] == outs[1][0] and outs[0][5] == outs[1][5] == 1
    assert all(same(outs[0][i], outs[1][i]) for i in (1, 2, 3, 4))
    assert not same(outs[0][1], p0)


# ---- 6. discarding -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_setter_discards_an_open_window(T):
    """small_plain: one micro-batch, then set_grad_accumulation(3) again -- the phase reads 0 and the next full window ends bit-identical
    (parameters, accumulator) to the same window on a net that never saw the discarded micro-batch"""
    from cnn_amd import hostapi

    layout = S.walk(SMALL_PLAIN, *PLAIN_SHAPE)
    p0 = he_init(layout, 650)
    B = 4
    mk = lambda i: (T.from_numpy(uniform01(651 + i, (B,) + PLAIN_SHAPE)).cuda(), T.from_numpy(((np.arange(B) + i) % 3).astype(np.int32)).cuda())
    stray, window = mk(0), [mk(i) for i in range(1, K + 1)]
    outs = []
    for discard in (True, False):
        net = hostapi.HostSequential(SMALL_PLAIN, PLAIN_SHAPE)
        net.set_params(p0)
        net.set_optimizer(0.9, 5e-4)
        net.set_grad_accumulation(K)
        if discard:
            net.train_step(*stray, LR)
            assert net.accumulation_phase() == 1 and same(net.get_params(), p0)
            net.set_grad_accumulation(K)
            assert net.accumulation_phase() == 0
        for j, (x, labels) in enumerate(window):
            net.train_step(x, labels, LR)
            assert net.accumulation_phase() == (j + 1) % K
        outs.append((net.get_params(), net.get_accumulated_grads(), net.get_velocity(), net.last_loss()))
        net.close()
    assert all(same(outs[0][i], outs[1][i]) for i in range(3)) and outs[0][3] == outs[1][3]
    assert not same(outs[0][0], p0)
