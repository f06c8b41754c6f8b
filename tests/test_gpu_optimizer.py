"""SGD with momentum / weight decay / Nesterov on the flat arena (cnn_sgd_momentum_update, Sequential::set_optimizer) on the device.
Every comparison is bit-exact (np.array_equal on the raw fp32): the reference (tests/optim_ref.py) is the same arithmetic."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

from cnn_amd import stacks as S
from tests.optim_ref import decay_ranges_of, moving_stat_mask, ref_sgd_step
from tests.util import he_init, uniform01

pytestmark = pytest.mark.gpu

ALEXNET_PARAMS = 111267  # the reference net's arena
PAD = 8                  # guard floats in front of and behind every test buffer


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_ranges(seed, n, count):
    """`count` (fewer when n is too small) sorted, disjoint, non-empty ranges at random cuts -- they start and end inside float4s --
    the last one ending at n"""
    count = min(count, (n + 1) // 2)
    if count == 0:
        return []
    rs = np.random.RandomState(seed)
    cuts = np.sort(rs.choice(n, size=2 * count - 1, replace=False)) if n >= 2 * count - 1 else np.arange(2 * count - 1)
    cuts = np.concatenate([cuts, [n]]).astype(np.int64)
    return [(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(count)]


class Buf:
    """n floats on the device between guard floats, 16-byte aligned or 4 bytes off"""

    def __init__(self, T, host, offset):
        self.n, self.start = host.size, PAD + (1 if offset else 0)
        full = np.full(host.size + 2 * PAD + 1, 12345.0, np.float32)
        full[self.start:self.start + self.n] = host
        self.full = T.from_numpy(full).cuda()
        self.view = self.full[self.start:self.start + self.n]
        assert (self.view.data_ptr() % 16 == 0) != bool(offset)

    def get(self):
        host = self.full.cpu().numpy()
        guard = np.concatenate([host[:self.start], host[self.start + self.n:]])
        assert np.all(guard == np.float32(12345.0)), "the kernel wrote outside its range"
        return host[self.start:self.start + self.n].copy()


def run_case(T, n, offset, grad_scale, n_ranges, with_prev, opt, seed, steps=3):
    from cnn_amd import capi

    momentum, wd, nesterov = opt
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    v = np.zeros(n, np.float32)
    ranges = make_ranges(seed + 1, n, n_ranges)
    off = (offset,) * 4 if isinstance(offset, bool) else offset
    pb, vb = Buf(T, p, off[0]), Buf(T, v, off[2])
    prevb = Buf(T, np.zeros(n, np.float32), off[3]) if with_prev else None
    lr = 0.05
    for step in range(steps):
        g = rs.standard_normal(n).astype(np.float32)
        gb = Buf(T, g, off[1])
        capi.sgd_momentum_update(pb.view, gb.view, vb.view, lr, momentum, wd, nesterov, grad_scale, ranges,
                                 prevb.view if with_prev else None)
        T.cuda.synchronize()
        want_p, want_v = ref_sgd_step(p, g, v, lr, momentum, wd, nesterov, grad_scale, ranges)
        tag = f"n={n} offset={offset} scale={grad_scale} ranges={len(ranges)} prev={with_prev} opt={opt} step={step}"
        assert same(pb.get(), want_p), "params: " + tag
        assert same(vb.get(), want_v), "velocity: " + tag
        assert same(gb.get(), g), "gradients changed: " + tag
        if with_prev:
            assert same(prevb.get(), p), "previous: " + tag
        p, v = want_p, want_v
    return ranges


OPTS = [(0.9, 5e-4, False), (0.9, 5e-4, True), (0.0, 5e-4, False), (0.9, 0.0, False)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, ALEXNET_PARAMS])
def test_kernel_equals_the_reference_step(T, n):
    """aligned and 4-byte-offset pointers, grad_scale 1 and 1/8, tables of 0 / 1 / 40 / 300 ranges (300: the device-table path) with
    ranges that start or end inside a float4 and one that ends at n, previous null and non-null, three steps so the velocity carries"""
    from cnn_amd import capi

    seed = 1000 + n
    seen = set()
    for offset in (False, True):
        for grad_scale in (1.0, 0.125):
            for n_ranges in (0, 1, 40, 300):
                for with_prev in (False, True):
                    for opt in OPTS:
                        seed += 1
                        seen.add(len(run_case(T, n, offset, grad_scale, n_ranges, with_prev, opt, seed)))
    if n >= 1023:
        assert max(seen) == 300 > capi.SGD_INLINE_RANGES and 40 in seen
    # one operand off alignment is enough for the scalar kernel: gradients only, velocity only
    run_case(T, n, (False, True, False, False), 0.125, 40, True, OPTS[1], seed + 1)
    run_case(T, n, (False, False, True, False), 1.0, 300, True, OPTS[0], seed + 2)


@pytest.mark.parametrize("offset,n_ranges,grad_scale,with_prev,opt", [(False, 300, 0.125, True, OPTS[1]), (True, 40, 1.0, False, OPTS[0]),
                                                                      (False, 1, 1.0, True, OPTS[0])])
def test_kernel_on_an_arena_beyond_2_pow_24(T, offset, n_ranges, grad_scale, with_prev, opt):
    """n = 2^24 + 5: element indices that fp32 could not hold, a grid-stride loop of several rounds, a scalar tail"""
    run_case(T, (1 << 24) + 5, offset, grad_scale, n_ranges, with_prev, opt, 77 + n_ranges, steps=3)


@pytest.mark.parametrize("n,offset", [(ALEXNET_PARAMS, False), (ALEXNET_PARAMS, True), (5, False), (4096, False)])
def test_momentum_0_and_decay_0_is_the_plain_step(T, n, offset):
    """through the new entry: cnn_sgd_update_keep's result bit for bit (parameters and `previous`), the velocity buffer -- pre-filled
    with a sentinel -- untouched; also with a decay table present (weight_decay 0 switches it off)"""
    from cnn_amd import capi

    lib = capi.load()
    rs = np.random.RandomState(5 + n)
    p, g = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    for grad_scale in (1.0, 0.125):
        for ranges in ([], make_ranges(3, n, 40)):
            a_p, a_prev = Buf(T, p, offset), Buf(T, np.zeros(n, np.float32), offset)
            b_p, b_prev = Buf(T, p, offset), Buf(T, np.zeros(n, np.float32), offset)
            gb, vb = Buf(T, g, offset), Buf(T, np.full(n, -3.25, np.float32), offset)
            capi.check(lib.cnn_sgd_update_keep(capi._ptr(a_p.view), capi._ptr(gb.view), n, 0.01, grad_scale, capi._ptr(a_prev.view), capi._stream()),
                       "cnn_sgd_update_keep")
            capi.sgd_momentum_update(b_p.view, gb.view, vb.view, 0.01, 0.0, 0.0, False, grad_scale, ranges, b_prev.view)
            T.cuda.synchronize()
            assert same(a_p.get(), b_p.get()) and same(a_prev.get(), b_prev.get()) and same(b_prev.get(), p)
            assert np.all(vb.get() == np.float32(-3.25)), "the velocity buffer was written"
            assert same(b_p.get(), ref_sgd_step(p, g, None, 0.01, grad_scale=grad_scale)[0])


def test_one_launch_per_call(T):
    """whatever the number of ranges: ONE kernel per call (the library's launch log: cnn_amd_kernel_timing_* with mode 1 records every
    launch) -- sgdm_vec for aligned pointers, its scalar tail riding in workgroup 0; sgdm_scalar alone for unaligned ones"""
    from cnn_amd import capi

    n = ALEXNET_PARAMS  # (not a multiple of 4: there is a tail)
    rs = np.random.RandomState(9)
    host = rs.standard_normal(n).astype(np.float32)
    for offset, kernel in ((False, "sgdm_vec"), (True, "sgdm_scalar")):
        for n_ranges in (0, 1, 40, 300):
            for momentum in (0.9, 0.0):
                p, g, v, prev = (Buf(T, host, offset) for _ in range(4))
                ranges = make_ranges(11, n, n_ranges)
                T.cuda.synchronize()
                capi.kernel_timing(1)
                capi.sgd_momentum_update(p.view, g.view, v.view, 0.01, momentum, 5e-4, False, 1.0, ranges, prev.view)
                rep = capi.kernel_timing_report()
                capi.kernel_timing(0)
                names = [(k.split("|")[0], cnt) for k, (cnt, _) in rep.items()]
                assert names == [(kernel, 1)], (offset, n_ranges, momentum, rep)


# ---- whole nets ------------------------------------------------------------------------------------------------------------------
SMALL_BN = [("conv", 8, 3, 1, 1), ("bn",), ("relu",), ("pool", 2, 2), ("conv", 16, 3, 1, 1), ("bn",), ("relu",), ("pool", 2, 2), ("linear", 3)]
NETS = {
    "alexnet": (S.alexnet(3), (3, 224, 224), 16),              # the reference net: pool-fused first block, fused step tail
    "alexnet_bn": (S.alexnet(3, batch_norm=True), (3, 224, 224), 8),  # AlexNet(3, true)
    "small_bn": (SMALL_BN, (3, 32, 32), 4),                    # BatchNorm + ReLU + MaxPool blocks, no pool-fused block at the front
}


def make_net(which):
    from cnn_amd import hostapi

    spec, in_shape, B = NETS[which]
    if which == "alexnet":
        return hostapi.HostAlexNet(3)
    if which == "alexnet_bn":
        return hostapi.HostAlexNet(3, batch_norm=True)
    return hostapi.HostSequential(spec, in_shape)


def net_inputs(T, which, seed):
    spec, in_shape, B = NETS[which]
    layout = S.walk(spec, *in_shape)
    p0 = he_init(layout, seed)
    x = T.from_numpy(uniform01(seed + 1, (B,) + in_shape)).cuda()
    labels = T.from_numpy((np.arange(B) % 3).astype(np.int32)).cuda()
    return layout, p0, x, labels


LR = 1e-2


def host_stepped_run(net, layout, p0, x, labels, opt, steps, bias_and_norm):
    """net B: forward -> device loss delta -> backward (the plain sequence, no step); the gradient arena comes back, ref_sgd_step runs on
    the host with the container's range table, the parameters go back through set_params (which calls parameters_changed())"""
    momentum, wd, nesterov = opt
    ranges = decay_ranges_of(layout, bias_and_norm)
    stats = moving_stat_mask(layout)
    net.set_params(p0)
    v = np.zeros(p0.size, np.float32)
    trace = []
    for _ in range(steps):
        net.forward_backward(x, labels)
        loss = net.last_loss()
        g = net.get_grads()
        p = net.get_params()  # (BatchNorm2D's forward pass moved the moving statistics)
        assert not np.any(g[stats]), "the gradient half of the moving statistics is zero"
        p_new, v = ref_sgd_step(p, g, v, LR, momentum, wd, nesterov, 1.0, ranges)
        assert same(p_new[stats], p[stats]) and not np.any(v[stats])
        net.set_params(p_new)
        trace.append((loss, p_new, v.copy(), p[stats].copy()))
    return trace


@pytest.mark.parametrize("variant", ["default", "nesterov_decay_bias_and_norm"])
@pytest.mark.parametrize("which", ["alexnet", "alexnet_bn", "small_bn"])
def test_train_step_with_optimizer_equals_host_stepped_net(T, which, variant):
    """net A: three train_steps with set_optimizer(0.9, 5e-4); net B: the plain sequence with the step done on the host.  Parameters,
    velocity and last_loss() agree bit for bit after every step; BatchNorm2D's moving statistics are what the forward passes alone
    produce, for both decay policies.  (Rests on the container's property that the fused tail's gradients are those of the plain
    sequence: a failure that shows with the optimizer off too is about the tail.)"""
    nesterov = bias_and_norm = variant != "default"
    opt = (0.9, 5e-4, nesterov)
    layout, p0, x, labels = net_inputs(T, which, 300)
    stats = moving_stat_mask(layout)
    assert stats.any() == (which != "alexnet")
    a, b = make_net(which), make_net(which)
    want = host_stepped_run(b, layout, p0, x, labels, opt, 3, bias_and_norm)
    a.set_params(p0)
    a.set_optimizer(*opt, decay_bias_and_norm=bias_and_norm)
    assert not np.any(a.get_velocity())
    for step, (loss, p, v, stats_after_forward) in enumerate(want):
        a.train_step(x, labels, LR)
        got_loss, got_p, got_v = a.last_loss(), a.get_params(), a.get_velocity()
        print(f"{which} {variant} step {step}: loss {got_loss!r} / {loss!r}, params differ at {int((bits(got_p) != bits(p)).sum())}, "
              f"velocity at {int((bits(got_v) != bits(v)).sum())} of {p.size}")
        assert got_loss == loss, (step, got_loss, loss)
        assert same(got_p, p), f"step {step}: parameters"
        assert same(got_v, v), f"step {step}: velocity"
        assert same(got_p[stats], stats_after_forward), f"step {step}: moving statistics"
    assert np.abs(want[-1][2]).max() > 0 and not same(want[-1][1], p0)
    a.close()
    b.close()


def test_plain_train_step_equals_host_stepped_net(T):
    """the same comparison with the optimizer OFF (momentum 0, weight decay 0 on the host side): what test_train_step_with_optimizer_...
    rests on -- the fused tail's gradients and the fused loss head are those of the plain sequence"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 300)
    a, b = make_net("alexnet"), make_net("alexnet")
    want = host_stepped_run(b, layout, p0, x, labels, (0.0, 0.0, False), 3, False)
    a.set_params(p0)
    for step, (loss, p, _, _) in enumerate(want):
        a.train_step(x, labels, LR)
        assert a.last_loss() == loss and same(a.get_params(), p), step
    a.close()
    b.close()


def test_get_output_after_an_optimizer_step(T):
    """a tensor the pool-fused pass did not write (the first block's Conv2D / ReLU outputs) is re-computed on demand from the snapshot
    of the parameters the pass used -- written by the new kernel's `previous` (arena behind the block) and by the block's own range
    step: after a step with the optimizer set it has the bits a pass that writes every tensor produces from the pre-step parameters"""
    from cnn_amd import hostapi

    layout, p0, x, labels = net_inputs(T, "alexnet", 310)
    B = x.shape[0]
    shapes = [("conv_layer_1", (16, 111, 111)), ("relu_layer_1", (16, 111, 111)), ("conv_layer_2", (32, 27, 27))]
    a = make_net("alexnet")
    a.set_params(p0)
    a.set_optimizer(0.9, 5e-4)
    for _ in range(2):
        a.train_step(x, labels, LR)
    before = a.get_params()  # the parameters step 3's forward pass uses
    a.train_step(x, labels, LR)  # (pool-fused, fused tail)
    got = [a.layer_output(name, (B,) + shp) for name, shp in shapes]
    assert not same(a.get_params(), before)
    a.close()
    lib = hostapi.load()
    ref = make_net("alexnet")
    ref.set_params(before)
    lib.cnnh_set_fuse_pool_block(0)
    try:
        ref.train_step(x, labels, LR)
        want = [ref.layer_output(name, (B,) + shp) for name, shp in shapes]
    finally:
        lib.cnnh_set_fuse_pool_block(1)
    ref.close()
    for (name, _), g, w in zip(shapes, got, want):
        assert same(g, w), name


def test_optimizer_state_round_trip(T, tmp_path):
    """weights + optimizer state saved after step 2 and loaded into a fresh net: step 3 is the uninterrupted run's, bit for bit; a
    state file written for another n_params is rejected and leaves the net as it was"""
    from cnn_amd import capi

    which = "alexnet_bn"
    layout, p0, x, labels = net_inputs(T, which, 320)
    opt = dict(momentum=0.9, weight_decay=5e-4, nesterov=True, decay_bias_and_norm=True)
    a = make_net(which)
    a.set_params(p0)
    a.set_optimizer(**opt)
    for _ in range(2):
        a.train_step(x, labels, LR)
    model, state = str(tmp_path / "step2.model"), str(tmp_path / "step2.optstate")
    a.save_checkpoint(model)
    a.save_optimizer_state(state)
    assert os.path.getsize(state) == 32 + 4 * a.n_params
    a.train_step(x, labels, LR)
    want = (a.last_loss(), a.get_params(), a.get_velocity())
    a.close()
    b = make_net(which)
    b.load_checkpoint(model)
    b.load_optimizer_state(state)  # (sets the options the file carries)
    b.train_step(x, labels, LR)
    got = (b.last_loss(), b.get_params(), b.get_velocity())
    assert got[0] == want[0] and same(got[1], want[1]) and same(got[2], want[2])
    # another n_params: rejected, nothing changed
    other = make_net("small_bn")
    assert other.n_params != b.n_params
    with pytest.raises(capi.CnnAmdError, match="n_params"):
        other.load_optimizer_state(state)
    assert not other.velocity_ptr()
    with pytest.raises(capi.CnnAmdError):
        other.save_optimizer_state(str(tmp_path / "none.optstate"))  # no optimizer was ever set
    other.close()
    truncated = str(tmp_path / "short.optstate")
    open(truncated, "wb").write(open(state, "rb").read()[:-8])
    before = b.get_velocity()
    with pytest.raises(capi.CnnAmdError):
        b.load_optimizer_state(truncated)
    with pytest.raises(FileNotFoundError):
        b.load_optimizer_state(str(tmp_path / "missing.optstate"))
    assert same(b.get_velocity(), before)
    b.close()


@pytest.mark.parametrize("which", ["alexnet", "alexnet_bn"])
def test_forced_one_rank_exchange_with_optimizer(T, which, lib_option):
    """the data-parallel branch of the fused tail (range steps behind the two all-reduce buckets) with the optimizer set, forced on with
    ONE rank (DP_FORCE_EXCHANGE: every sum is an identity): parameters and velocity of four steps equal the no-communicator run's"""
    from cnn_amd.dp import RcclComm

    layout, p0, x, labels = net_inputs(T, which, 330)
    comm = RcclComm(None, 1, 0)
    outs = []
    for use_comm in (False, True):
        net = make_net(which)
        net.set_params(p0)
        net.set_optimizer(0.9, 5e-4)
        if use_comm:
            net.set_comm(comm.handle, 1)
            lib_option("DP_FORCE_EXCHANGE", "1")
        losses = []
        for _ in range(4):
            net.train_step(x, labels, LR)
            losses.append(net.last_loss())
        outs.append((losses, net.get_params(), net.get_velocity()))
        net.close()
        lib_option("DP_FORCE_EXCHANGE", None)
    comm.destroy()
    assert outs[0][0] == outs[1][0]
    assert same(outs[0][1], outs[1][1]) and same(outs[0][2], outs[1][2])


def test_two_replicas_with_optimizer(T):
    """two replicas of the C++ container (one per GPU, ncclCommInitAll) with the optimizer set, each on half of the batch: the
    all-reduced gradient is the same on every rank, so parameters AND velocities stay identical without any exchange of the velocity;
    against one replica on the whole batch they differ by summation order only (the bound of the existing two-replica test)"""
    world = 2
    if T.cuda.device_count() < world:
        pytest.skip("needs two GPUs (the driver's 1-GPU test box has one)")
    from cnn_amd import capi, hostapi

    lib = capi.load()
    spec, in_shape, GB = S.alexnet(3, batch_norm=True), (3, 224, 224), 8
    p0 = he_init(S.walk(spec, *in_shape), 91)
    steps, half = 2, GB // world
    x = uniform01(92, (GB,) + in_shape)
    labels = (np.arange(GB) % 3).astype(np.int32)
    comms = (C.c_void_p * world)()
    capi.check(lib.cnn_comm_init_all(comms, world, None), "cnn_comm_init_all")
    results, errors = [None] * world, []

    def replica(rank):
        try:
            T.cuda.set_device(rank)
            xs = T.from_numpy(x[rank * half:(rank + 1) * half]).cuda()
            ls = T.from_numpy(labels[rank * half:(rank + 1) * half]).cuda()
            net = hostapi.HostSequential(spec, in_shape)
            net.set_params(p0)
            net.set_optimizer(0.9, 5e-4)
            net.set_comm(C.c_void_p(comms[rank]), world)
            for _ in range(steps):
                net.train_step(xs, ls, 1e-3)
            T.cuda.synchronize()
            results[rank] = (net.get_params(), net.get_velocity())
            net.close()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=replica, args=(r,)) for r in range(world)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    T.cuda.set_device(0)
    full = hostapi.HostSequential(spec, in_shape)
    full.set_params(p0)
    full.set_optimizer(0.9, 5e-4)
    xf, lf = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    for _ in range(steps):
        full.train_step(xf, lf, 1e-3)
    want = full.get_params()
    full.close()
    for c in comms:
        lib.cnn_comm_destroy(C.c_void_p(c))
    assert same(results[0][0], results[1][0]) and same(results[0][1], results[1][1]), "replicas diverged"
    err = np.abs(results[0][0] - want).max() / np.abs(want).max()
    assert err <= 1e-5, err


def step_kernels(T, net, x, labels, steps=3):
    from cnn_amd import capi

    T.cuda.synchronize()
    capi.kernel_timing(1)
    for _ in range(steps):
        net.train_step(x, labels, 1e-3)
    net.flush()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    return {k: cnt for k, (cnt, _) in rep.items()}


def test_default_path_is_untouched(T, golden_dir):
    """without set_optimizer -- and after set_optimizer(0, 0) -- three train_steps of the reference net at B = 16 launch exactly the
    kernels ("<kernel>|<geometry>" -> launches, from the library's launch log) that the commit before the optimizer launched
    (tests/golden/train_step_kernels_before_optimizer.json, recorded from that commit's library), none of them the optimizer's, and
    end with the same parameters; with the optimizer set the arena's step is sgdm_vec and the block's in-kernel step is gone.
    The golden file pins every kernel of the default step: a change that alters them on purpose (a rename, a retune, another fusion)
    re-records it with tests/golden/make_train_step_kernels.py and commits the new file."""
    layout, p0, x, labels = net_inputs(T, "alexnet", 340)
    golden = json.load(open(os.path.join(golden_dir, "train_step_kernels_before_optimizer.json")))
    runs = {}
    for mode in ("never", "off_again", "on"):
        net = make_net("alexnet")
        net.set_params(p0)
        if mode != "never":
            net.set_optimizer(0.9, 5e-4)
        if mode == "off_again":
            net.set_optimizer(0, 0)
        runs[mode] = (step_kernels(T, net, x, labels), net.get_params())
        net.close()
    assert runs["never"][0] == golden, sorted(set(runs["never"][0].items()) ^ set(golden.items()))
    assert runs["off_again"][0] == golden and same(runs["never"][1], runs["off_again"][1])
    assert not any(k.startswith("sgdm") for k in golden)
    on = runs["on"][0]
    assert sum(cnt for k, cnt in on.items() if k.startswith("sgdm_vec|")) == 1 + 2 * 2  # step 1: the arena; steps 2, 3: two ranges each
    assert not any(k.startswith("sgd_vec") or k.startswith("sgd_scalar") for k in on)
    assert not same(runs["on"][1], runs["never"][1])
