"""Adam / AdamW (cnn_adam_update, Sequential::set_adam) and the clip by the global gradient norm (cnn_clip_grad_norm,
Sequential::set_grad_clip) on the device.  Every comparison of parameters and state is bit-exact (np.array_equal on the raw fp32):
the reference (tests/adam_ref.py) is the same arithmetic.  The total norm alone is held to an fp64 NumPy value with one fp32 ulp of
allowance for a rounding tie."""
import json
import os

import numpy as np
import pytest

from tests.adam_ref import ref_adam_step, ref_clip, ref_total_norm
from tests.optim_ref import decay_ranges_of, moving_stat_mask, ref_sgd_step
from tests.test_gpu_optimizer import ALEXNET_PARAMS, Buf, bits, make_net, make_ranges, net_inputs, same, step_kernels

pytestmark = pytest.mark.gpu

LR = 1e-3
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def sparse_normal(rs, n):
    """standard-normal gradients with every 97th exactly 0 (a zero gradient on a zero state must leave the parameter alone)"""
    g = rs.standard_normal(n).astype(np.float32)
    g[::97] = 0.0
    return g


def run_case(T, n, offset, grad_scale, n_ranges, with_prev, opt, seed, steps=(1, 2, 3)):
    """`steps`: the step numbers handed to consecutive calls; both moments carry over from call to call"""
    from cnn_amd import capi

    wd, decoupled = opt
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    ranges = make_ranges(seed + 1, n, n_ranges)
    off = (offset,) * 5 if isinstance(offset, bool) else offset
    pb, mb, vb = Buf(T, p, off[0]), Buf(T, m, off[2]), Buf(T, v, off[3])
    prevb = Buf(T, np.zeros(n, np.float32), off[4]) if with_prev else None
    for step in steps:
        g = sparse_normal(rs, n)
        gb = Buf(T, g, off[1])
        capi.adam_update(pb.view, gb.view, mb.view, vb.view, LR, ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, decoupled, step, grad_scale,
                         ranges, prevb.view if with_prev else None)
        T.cuda.synchronize()
        want_p, want_m, want_v = ref_adam_step(p, g, m, v, step, LR, ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, decoupled, grad_scale, ranges)
        tag = f"n={n} offset={offset} scale={grad_scale} ranges={len(ranges)} prev={with_prev} opt={opt} step={step}"
        got_p, got_m, got_v = pb.get(), mb.get(), vb.get()
        if not (same(got_p, want_p) and same(got_m, want_m) and same(got_v, want_v)):
            print(tag, "differing words: p", int((bits(got_p) != bits(want_p)).sum()), "m", int((bits(got_m) != bits(want_m)).sum()), "v",
                  int((bits(got_v) != bits(want_v)).sum()))
        assert same(got_p, want_p), "params: " + tag
        assert same(got_m, want_m), "exp_avg: " + tag
        assert same(got_v, want_v), "exp_avg_sq: " + tag
        assert same(gb.get(), g), "gradients changed: " + tag
        if with_prev:
            assert same(prevb.get(), p), "previous: " + tag
        p, m, v = want_p, want_m, want_v
    return ranges


OPTS = [(0.0, False), (1e-2, False), (0.0, True), (1e-2, True)]  # (weight decay, decoupled)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, ALEXNET_PARAMS])
def test_kernel_equals_the_reference_step(T, n):
    """aligned and 4-byte-offset pointers, grad_scale 1 and 1/8, tables of 0 / 1 / 40 / 300 ranges (300: the device-table path) with
    ranges that start or end inside a float4 and one that ends at n, previous null and non-null, Adam and AdamW with and without
    decay, steps 1, 2, 3 so that both moments carry; guard floats intact, gradients unchanged"""
    from cnn_amd import capi

    seed = 2000 + n
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
    # one operand off alignment is enough for the scalar kernel: exp_avg_sq only, `previous` only
    run_case(T, n, (False, False, False, True, False), 0.125, 40, True, OPTS[1], seed + 1)
    run_case(T, n, (False, False, False, False, True), 1.0, 300, True, OPTS[3], seed + 2)
    # step 1000: both bias corrections are near 1
    run_case(T, n, False, 1.0, 40, True, OPTS[1], seed + 3, steps=(1000, 1001))


@pytest.mark.parametrize("offset,n_ranges,grad_scale,with_prev,opt", [(False, 300, 0.125, True, OPTS[3]), (True, 40, 1.0, False, OPTS[1])])
def test_kernel_on_an_arena_beyond_2_pow_24(T, offset, n_ranges, grad_scale, with_prev, opt):
    """n = 2^24 + 5: element indices that fp32 could not hold, a grid-stride loop of several rounds, a scalar tail"""
    run_case(T, (1 << 24) + 5, offset, grad_scale, n_ranges, with_prev, opt, 177 + n_ranges, steps=(1, 2))


def test_one_launch_per_call(T):
    """whatever the number of ranges: ONE kernel per call (the library's launch log) -- adam_vec for aligned pointers, its scalar tail
    riding in workgroup 0; adam_scalar alone for unaligned ones"""
    from cnn_amd import capi

    n = ALEXNET_PARAMS  # (not a multiple of 4: there is a tail)
    rs = np.random.RandomState(9)
    host = np.abs(rs.standard_normal(n).astype(np.float32))
    for offset, kernel in ((False, "adam_vec"), (True, "adam_scalar")):
        for n_ranges in (0, 1, 40, 300):
            for decoupled in (False, True):
                p, g, m, v, prev = (Buf(T, host, offset) for _ in range(5))
                ranges = make_ranges(11, n, n_ranges)
                T.cuda.synchronize()
                capi.kernel_timing(1)
                capi.adam_update(p.view, g.view, m.view, v.view, LR, weight_decay=1e-2, decoupled=decoupled, step=2, decay_ranges=ranges,
                                 previous=prev.view)
                rep = capi.kernel_timing_report()
                capi.kernel_timing(0)
                names = [(k.split("|")[0], cnt) for k, (cnt, _) in rep.items()]
                assert names == [(kernel, 1)], (offset, n_ranges, decoupled, rep)


# ---- the clip kernel ---------------------------------------------------------------------------------------------------------------
def clip_sizes():
    """... and one n at which EVERY workgroup of the largest grid the clip kernels launch takes more than one grid-stride round: the
    grid never exceeds CLIP_MAX_BLOCKS workgroups of CLIP_BLOCK lanes, the vector kernels take a float4 per lane and round, so one
    round of the largest grid covers CLIP_MAX_BLOCKS * CLIP_BLOCK * 4 floats; two full rounds and an odd tail of 5"""
    from cnn_amd import capi

    return [1, 5, 1023, ALEXNET_PARAMS, 2 * capi.CLIP_MAX_BLOCKS * capi.CLIP_BLOCK * 4 + 5]


def ulp_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.uint32)) - int(b.view(np.uint32)))  # (both positive and finite here)


@pytest.mark.parametrize("index", range(5))
def test_clip_kernel(T, index):
    """stats[0] is the fp64 NumPy norm (times grad_scale in fp32) or its fp32 neighbour; the coefficient and the scaled gradients are
    ref_clip from the device's own stats[0], bit for bit; two calls on the same data give identical words; max_norm = 2 x norm and a
    NaN gradient leave the buffer's words alone with a coefficient of exactly 1"""
    from cnn_amd import capi

    n = clip_sizes()[index]
    rs = np.random.RandomState(50 + index)
    g = sparse_normal(rs, n)
    if n == 1:
        g[0] = np.float32(1.7)
    used_allowance = cases = 0
    for offset in (False, True):
        for grad_scale in (1.0, 0.125):
            want_total = ref_total_norm(g, grad_scale)
            runs = []
            for _ in range(2):
                gb = Buf(T, g, offset)
                stats = capi.clip_grad_norm(gb.view, 0.5 * float(want_total), grad_scale).cpu().numpy()
                runs.append((stats, gb.get()))
            (stats, got), (stats2, got2) = runs
            tag = f"n={n} offset={offset} scale={grad_scale}"
            assert same(stats, stats2) and same(got, got2), "two runs differ: " + tag
            apart = ulp_apart(stats[0], want_total)
            print(f"{tag}: total {stats[0]!r} want {want_total!r} ({apart} ulp apart), coef {stats[1]!r}")
            assert apart <= 1, tag
            cases += 1
            used_allowance += apart
            want_g, want_coef = ref_clip(g, stats[0], 0.5 * float(want_total))
            assert want_coef < 1 and bits(stats[1:2])[0] == bits(np.asarray([want_coef]))[0], tag
            assert same(got, want_g), "scaled gradients: " + tag
            # no clipping: the coefficient is exactly 1 and the buffer keeps its words
            gb = Buf(T, g, offset)
            stats = capi.clip_grad_norm(gb.view, 2.0 * float(want_total), grad_scale).cpu().numpy()
            assert stats[1] == np.float32(1) and ulp_apart(stats[0], want_total) <= 1 and same(gb.get(), g), tag
            # one NaN gradient: NaN total, coefficient 1, buffer unchanged
            bad = g.copy()
            bad[n // 2] = np.float32("nan")
            gb = Buf(T, bad, offset)
            stats = capi.clip_grad_norm(gb.view, 1.0, grad_scale).cpu().numpy()
            assert np.isnan(stats[0]) and stats[1] == np.float32(1) and same(gb.get(), bad), tag
    print(f"n={n}: {used_allowance} of {cases} cases used the one-ulp allowance")


def test_clip_launches(T):
    """at most three launches per call, named in the library's launch log: the partial sums, the ordered finish, the scaling pass"""
    from cnn_amd import capi

    g = sparse_normal(np.random.RandomState(8), ALEXNET_PARAMS)
    for offset, kind in ((False, "vec"), (True, "scalar")):
        gb = Buf(T, g, offset)
        T.cuda.synchronize()
        capi.kernel_timing(1)
        capi.clip_grad_norm(gb.view, 1.0)
        rep = capi.kernel_timing_report()
        capi.kernel_timing(0)
        names = sorted((k.split("|")[0], cnt) for k, (cnt, _) in rep.items())
        assert names == sorted([("clip_partial_" + kind, 1), ("clip_finish", 1), ("clip_scale_" + kind, 1)]), rep


# ---- whole nets ------------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "adam_l2": dict(weight_decay=1e-2, decoupled=False, decay_bias_and_norm=False),
    "adamw_decay_bias_and_norm": dict(weight_decay=1e-2, decoupled=True, decay_bias_and_norm=True),
}


def host_adam_step(layout, opt, p, g, m, v, step, grad_scale=1.0):
    ranges = decay_ranges_of(layout, opt["decay_bias_and_norm"])
    return ref_adam_step(p, g, m, v, step, LR, ADAM["beta1"], ADAM["beta2"], ADAM["eps"], opt["weight_decay"], opt["decoupled"], grad_scale, ranges)


def host_stepped_adam_run(net, layout, p0, x, labels, opt, steps):
    """net B: forward -> device loss delta -> backward (the plain sequence, no step); the gradient arena comes back, ref_adam_step runs
    on the host with the container's range table, the parameters go back through set_params"""
    stats = moving_stat_mask(layout)
    net.set_params(p0)
    m, v = np.zeros(p0.size, np.float32), np.zeros(p0.size, np.float32)
    trace = []
    for step in range(1, steps + 1):
        net.forward_backward(x, labels)
        loss = net.last_loss()
        g = net.get_grads()
        p = net.get_params()  # (BatchNorm2D's forward pass moved the moving statistics)
        assert not np.any(g[stats]), "the gradient half of the moving statistics is zero"
        p_new, m, v = host_adam_step(layout, opt, p, g, m, v, step)
        assert same(p_new[stats], p[stats]) and not np.any(m[stats]) and not np.any(v[stats])
        net.set_params(p_new)
        trace.append((loss, p_new, m.copy(), v.copy(), p[stats].copy()))
    return trace


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("which", ["alexnet", "alexnet_bn", "small_bn"])
def test_train_step_with_adam_equals_host_stepped_net(T, which, variant):
    """net A: set_adam and three train_steps; net B: the plain sequence with ref_adam_step on the host.  Parameters, both moments and
    last_loss() agree bit for bit after every step, BatchNorm2D's moving statistics are what the forward passes alone produce, and
    the step counter counts container steps -- 3, although the fused tail launches the step kernel twice per step"""
    opt = VARIANTS[variant]
    layout, p0, x, labels = net_inputs(T, which, 400)
    stats = moving_stat_mask(layout)
    a, b = make_net(which), make_net(which)
    want = host_stepped_adam_run(b, layout, p0, x, labels, opt, 3)
    a.set_params(p0)
    a.set_adam(**ADAM, **opt)
    m0, v0, t0 = a.get_adam_state()
    assert not np.any(m0) and not np.any(v0) and t0 == 0
    for step, (loss, p, m, v, stats_after_forward) in enumerate(want):
        a.train_step(x, labels, LR)
        got_loss, got_p = a.last_loss(), a.get_params()
        got_m, got_v, got_t = a.get_adam_state()
        print(f"{which} {variant} step {step}: loss {got_loss!r} / {loss!r}, params differ at {int((bits(got_p) != bits(p)).sum())}, "
              f"exp_avg at {int((bits(got_m) != bits(m)).sum())}, exp_avg_sq at {int((bits(got_v) != bits(v)).sum())} of {p.size}")
        assert got_loss == loss, (step, got_loss, loss)
        assert same(got_p, p), f"step {step}: parameters"
        assert same(got_m, m) and same(got_v, v), f"step {step}: moments"
        assert same(got_p[stats], stats_after_forward), f"step {step}: moving statistics"
        assert got_t == step + 1
    assert a.get_adam_state()[2] == 3
    assert np.abs(want[-1][2]).max() > 0 and not same(want[-1][1], p0)
    a.close()
    b.close()


def test_fused_tail_launches_the_adam_kernel_twice_per_step(T):
    """the reference net at B = 16: step 1 steps the whole arena, steps 2 and 3 run the fused tail with two range launches each -- five
    adam_vec launches, a step counter of 3, and none of the other step kernels"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 340)
    net = make_net("alexnet")
    net.set_params(p0)
    net.set_adam()
    log = step_kernels(T, net, x, labels)
    assert sum(cnt for k, cnt in log.items() if k.startswith("adam_vec|")) == 1 + 2 * 2, log
    assert not any(k.startswith(("sgd_vec", "sgd_scalar", "sgdm_", "adam_scalar", "clip_")) for k in log)
    assert net.get_adam_state()[2] == 3
    net.close()


def test_get_output_after_an_adam_step(T):
    """a tensor the pool-fused pass did not write is re-computed on demand from the snapshot of the parameters the pass used --
    written through adam_vec's `previous`: after an Adam step it has the bits a pass that writes every tensor produces from the
    pre-step parameters"""
    from cnn_amd import hostapi

    layout, p0, x, labels = net_inputs(T, "alexnet", 410)
    B = x.shape[0]
    shapes = [("conv_layer_1", (16, 111, 111)), ("relu_layer_1", (16, 111, 111)), ("conv_layer_2", (32, 27, 27))]
    a = make_net("alexnet")
    a.set_params(p0)
    a.set_adam(weight_decay=1e-2)
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


# ---- clipping in the container -----------------------------------------------------------------------------------------------------
SGD = (0.9, 5e-4, False)


def arm(net, optimizer):
    if optimizer == "sgdm":
        net.set_optimizer(*SGD)
    elif optimizer == "adam":
        net.set_adam(**ADAM, **VARIANTS["adam_l2"])


@pytest.mark.parametrize("optimizer", ["plain", "sgdm", "adam"])
def test_clipping_in_the_container(T, optimizer):
    """net A clips (max_norm = half the fp64 norm of step 1's gradient, so that clipping engages) and steps on the device; net B
    supplies every step's gradient through the plain sequence and takes the host step on ref_clip(g, A's device norm).  A's norm is
    within one fp32 ulp of the fp64 norm of B's gradient, coefficient and parameters agree bit for bit"""
    which = "alexnet"
    layout, p0, x, labels = net_inputs(T, which, 420)
    a, b = make_net(which), make_net(which)
    a.set_params(p0)
    b.set_params(p0)
    arm(a, optimizer)
    state = [np.zeros(p0.size, np.float32), np.zeros(p0.size, np.float32)]  # velocity, or the two moments
    max_norm = None
    for step in range(1, 4):
        b.forward_backward(x, labels)
        g, p = b.get_grads(), b.get_params()
        norm64 = ref_total_norm(g)
        if max_norm is None:
            max_norm = 0.5 * float(norm64)
            a.set_grad_clip(max_norm)
        a.train_step(x, labels, LR)
        norm, coef = a.last_grad_norm()
        print(f"{optimizer} step {step}: device norm {norm!r}, fp64 norm {norm64!r}, coefficient {coef!r}")
        assert ulp_apart(norm, norm64) <= 1, step
        g_clipped, want_coef = ref_clip(g, norm, max_norm)
        assert bits(np.asarray([coef]))[0] == bits(np.asarray([want_coef]))[0]
        if step == 1:
            assert coef < 1
        if optimizer == "plain":
            p_new = ref_sgd_step(p, g_clipped, None, LR)[0]
        elif optimizer == "sgdm":
            p_new, state[0] = ref_sgd_step(p, g_clipped, state[0], LR, *SGD, 1.0, decay_ranges_of(layout, False))
        else:
            p_new, state[0], state[1] = host_adam_step(layout, VARIANTS["adam_l2"], p, g_clipped, state[0], state[1], step)
        assert a.last_loss() == b.last_loss()
        assert same(a.get_params(), p_new), f"{optimizer} step {step}: parameters"
        b.set_params(p_new)
    a.close()
    b.close()


@pytest.mark.parametrize("optimizer", ["plain", "adam"])
def test_a_clip_that_never_engages_changes_nothing_and_switching_it_off_restores_the_fused_tail(T, optimizer):
    """max_norm = 1e30: three steps equal an unclipped net's bit for bit (the clipped net takes the plain sequence, the other the fused
    tail); after set_grad_clip(0) -- and one step that re-prepares the filter images -- the launch log of three further steps equals
    that of the net that never clipped: the fused tail is back"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 430)
    nets = {}
    for name in ("never", "clipped"):
        net = make_net("alexnet")
        net.set_params(p0)
        arm(net, optimizer)
        if name == "clipped":
            net.set_grad_clip(1e30)
        for _ in range(3):
            net.train_step(x, labels, LR)
        nets[name] = net
    assert nets["clipped"].last_grad_norm()[1] == np.float32(1)
    assert nets["never"].last_loss() == nets["clipped"].last_loss()
    assert same(nets["never"].get_params(), nets["clipped"].get_params())
    during = step_kernels(T, nets["clipped"], x, labels, steps=1)
    assert sum(cnt for k, cnt in during.items() if k.startswith("clip_")) == 3, during
    nets["clipped"].set_grad_clip(0)
    # one settling step each: the step behind a plain sequence re-prepares every filter image, as after any update_gradients()
    # (the learning rate is step_kernels': the two nets stay in step)
    nets["clipped"].train_step(x, labels, 1e-3)
    for _ in range(2):
        nets["never"].train_step(x, labels, 1e-3)
    logs = {name: step_kernels(T, net, x, labels) for name, net in nets.items()}
    assert logs["clipped"] == logs["never"], sorted(set(logs["clipped"].items()) ^ set(logs["never"].items()))
    assert not any(k.startswith("clip_") for k in logs["clipped"])
    assert same(nets["never"].get_params(), nets["clipped"].get_params())
    for net in nets.values():
        net.close()


# ---- state file, exchange, switching ------------------------------------------------------------------------------------------------
def test_adam_state_round_trip(T, tmp_path):
    """weights + Adam state saved after step 2 and loaded into a fresh net: step 3 is the uninterrupted run's, bit for bit.  An SGD
    state file still loads and activates SGD; a file for another n_params is status 3, a truncated Adam file status 2, and neither
    changes anything"""
    from cnn_amd import capi

    which = "alexnet_bn"
    layout, p0, x, labels = net_inputs(T, which, 440)
    opt = dict(ADAM, **VARIANTS["adamw_decay_bias_and_norm"])
    a = make_net(which)
    a.set_params(p0)
    a.set_adam(**opt)
    for _ in range(2):
        a.train_step(x, labels, LR)
    model, state = str(tmp_path / "step2.model"), str(tmp_path / "step2.adamstate")
    a.save_checkpoint(model)
    a.save_optimizer_state(state)
    assert os.path.getsize(state) == 48 + 2 * 4 * a.n_params and open(state, "rb").read(8) == b"CNNAADM1"
    a.train_step(x, labels, LR)
    want = (a.last_loss(), a.get_params()) + a.get_adam_state()
    b = make_net(which)
    b.load_checkpoint(model)
    b.load_optimizer_state(state)  # (sets the options and the step counter the file carries)
    assert b.get_adam_state()[2] == 2
    b.train_step(x, labels, LR)
    got = (b.last_loss(), b.get_params()) + b.get_adam_state()
    assert got[0] == want[0] and same(got[1], want[1]) and same(got[2], want[2]) and same(got[3], want[3]) and got[4] == want[4] == 3
    # an SGD state file loads into the net that runs Adam and activates SGD: the next state file is the SGD format again
    sgd_state, again = str(tmp_path / "sgd.optstate"), str(tmp_path / "again.optstate")
    a.set_optimizer(0.9, 5e-4)
    a.train_step(x, labels, LR)
    a.save_optimizer_state(sgd_state)
    assert open(sgd_state, "rb").read(8) == b"CNNAOPT1" and os.path.getsize(sgd_state) == 32 + 4 * a.n_params
    velocity = a.get_velocity()
    a.close()
    b.load_optimizer_state(sgd_state)
    assert same(b.get_velocity(), velocity)
    b.save_optimizer_state(again)
    assert open(again, "rb").read() == open(sgd_state, "rb").read()
    assert same(b.get_adam_state()[0], got[2]) and b.get_adam_state()[2] == 3  # (the moments survive the switch)
    b.load_optimizer_state(state)
    b.save_optimizer_state(again)
    assert open(again, "rb").read() == open(state, "rb").read()
    # another n_params: status 3, nothing changed
    other = make_net("small_bn")
    assert other.n_params != b.n_params
    with pytest.raises(capi.CnnAmdError, match="n_params"):
        other.load_optimizer_state(state)
    assert other.adam_ptrs() == (None, None)
    assert other.lib.cnnh_net_load_optimizer_state(other.h, state.encode()) == 3
    other.close()
    # truncated: status 2, nothing changed
    truncated = str(tmp_path / "short.adamstate")
    open(truncated, "wb").write(open(state, "rb").read()[:-8])
    before = b.get_adam_state()
    assert b.lib.cnnh_net_load_optimizer_state(b.h, truncated.encode()) == 2
    header_only = str(tmp_path / "header.adamstate")
    open(header_only, "wb").write(open(state, "rb").read()[:40])
    assert b.lib.cnnh_net_load_optimizer_state(b.h, header_only.encode()) == 2
    after = b.get_adam_state()
    assert same(before[0], after[0]) and same(before[1], after[1]) and before[2] == after[2]
    b.close()


@pytest.mark.parametrize("which", ["alexnet", "alexnet_bn"])
def test_forced_one_rank_exchange_with_adam_and_clipping(T, which, lib_option):
    """the data-parallel route (all-reduce, clip, step) with Adam and clipping on, forced on with ONE rank (DP_FORCE_EXCHANGE: every sum
    is an identity): parameters, moments and norms of four steps equal the no-communicator run's"""
    from cnn_amd.dp import RcclComm

    layout, p0, x, labels = net_inputs(T, which, 450)
    probe = make_net(which)
    probe.set_params(p0)
    probe.forward_backward(x, labels)
    max_norm = 0.5 * float(ref_total_norm(probe.get_grads()))
    probe.close()
    comm = RcclComm(None, 1, 0)
    outs = []
    for use_comm in (False, True):
        net = make_net(which)
        net.set_params(p0)
        net.set_adam(**ADAM, **VARIANTS["adam_l2"])
        net.set_grad_clip(max_norm)
        if use_comm:
            net.set_comm(comm.handle, 1)
            lib_option("DP_FORCE_EXCHANGE", "1")
        losses, norms = [], []
        for _ in range(4):
            net.train_step(x, labels, LR)
            losses.append(net.last_loss())
            norms.append(tuple(float(s) for s in net.last_grad_norm()))
        outs.append((losses, norms, net.get_params()) + net.get_adam_state())
        net.close()
        lib_option("DP_FORCE_EXCHANGE", None)
    comm.destroy()
    assert outs[0][1][0][1] < 1  # (clipping engaged at step 1)
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] and outs[0][5] == outs[1][5] == 4
    assert same(outs[0][2], outs[1][2]) and same(outs[0][3], outs[1][3]) and same(outs[0][4], outs[1][4])


def test_switching_between_the_optimizers(T):
    """set_adam -> set_optimizer(0.9, 5e-4) -> set_adam: the moments and the step counter survive the momentum steps in between, the
    velocity survives the Adam steps the other way round; no state arena is freed or zeroed by a switch"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 460)
    net = make_net("alexnet")
    net.set_params(p0)
    net.set_adam()
    for _ in range(2):
        net.train_step(x, labels, LR)
    m2, v2, t2 = net.get_adam_state()
    assert t2 == 2 and np.any(m2) and np.any(v2)
    net.set_optimizer(0.9, 5e-4)
    assert not np.any(net.get_velocity())
    net.train_step(x, labels, LR)
    vel = net.get_velocity()
    m, v, t = net.get_adam_state()
    assert np.any(vel) and same(m, m2) and same(v, v2) and t == 2
    net.set_adam()
    m, v, t = net.get_adam_state()
    assert same(m, m2) and same(v, v2) and t == 2
    net.train_step(x, labels, LR)
    m, v, t = net.get_adam_state()
    assert t == 3 and not same(m, m2) and same(net.get_velocity(), vel)
    net.close()


def test_plain_step_after_adam_is_the_default_path(T, golden_dir):
    """set_adam, then set_optimizer(0, 0): three train_steps of the reference net launch exactly the kernels of the commit before the
    optimizers (tests/golden/train_step_kernels_before_optimizer.json, at that test's inputs) and end with the parameters of a net
    that never had an optimizer"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 340)
    golden = json.load(open(os.path.join(golden_dir, "train_step_kernels_before_optimizer.json")))
    runs = {}
    for mode in ("never", "adam_then_plain"):
        net = make_net("alexnet")
        net.set_params(p0)
        if mode != "never":
            net.set_adam(weight_decay=1e-2)
            net.set_grad_clip(1.0)
            net.set_grad_clip(0)
            net.set_optimizer(0, 0)
        runs[mode] = (step_kernels(T, net, x, labels), net.get_params())
        if mode != "never":
            assert net.get_adam_state()[2] == 0
        net.close()
    assert runs["never"][0] == golden
    assert runs["adam_then_plain"][0] == golden, sorted(set(runs["adam_then_plain"][0].items()) ^ set(golden.items()))
    assert same(runs["never"][1], runs["adam_then_plain"][1])
    assert not any(k.startswith(("adam", "clip", "sgdm")) for k in golden)
