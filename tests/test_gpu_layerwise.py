"""LAMB and LARS on the flat arena (cnn_segment_norms, cnn_lamb_update, cnn_lars_update, Sequential::set_lamb / set_lars) on the
device.  The segment norms are held to the fp64 NumPy norm with one fp32 ulp of allowance (the fp64 sums differ only in their
order: ~1e-13 relative against a half-ulp of 6e-8, so only a rounding tie can differ); everything behind the norms -- ratios,
parameters, state, `update`, `previous` -- is compared bit for bit with the reference (tests/lamb_ref.py) evaluated from the
device's own norms."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from cnn_amd import stacks as S
from tests.adam_ref import ref_clip, ref_total_norm
from tests.lamb_ref import (SEG_ADAPT, SEG_DECAY, ref_lamb_moments, ref_lamb_step, ref_lars_step, ref_segment_norms, segment_table_of)
from tests.optim_ref import moving_stat_mask, ref_sgd_step
from tests.test_gpu_optimizer import NETS, Buf, bits, make_net, net_inputs, same, step_kernels

pytestmark = pytest.mark.gpu

ALEXNET_PARAMS = 111267
BIG = (1 << 24) + 5
LR = 1e-2
ALLOWANCE_USED = {"norms": 0, "of": 0}  # how many norms sat on the fp32 neighbour of the NumPy value (printed by the tests)


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.uint32).astype(np.int64) - b.view(np.uint32).astype(np.int64))  # (non-negative finite values)


def norms_close(got, want, tag):
    d = ulps(got, want)
    ALLOWANCE_USED["norms"] += int((d == 1).sum())
    ALLOWANCE_USED["of"] += int(d.size)
    assert np.all(d <= 1), f"{tag}: a norm is {int(d.max())} ulps from the fp64 value"


def make_table(kind, n, seed):
    """bounds of the segment table `kind` over [0, n)"""
    rs = np.random.RandomState(seed)
    if kind == "one" or n == 1:
        cuts = []
    elif kind == "seven":
        cuts = rs.choice(np.arange(1, n), min(6, n - 1), replace=False)
    elif kind == "300":
        assert n >= 1023
        cuts = set(rs.choice(np.arange(1, n), 280, replace=False).tolist())
        for c in rs.choice(np.arange(8, n - 8), 400, replace=False).tolist():  # segments of length 1, bounds inside a float4
            if len(cuts) >= 299:
                break
            cuts.add(int(c) | 1)
            if len(cuts) < 299:
                cuts.add((int(c) | 1) + 1)
        cuts = sorted(cuts)[:299]
    elif kind == "each":
        cuts = np.arange(1, n)
    elif kind == "net":
        assert n == ALEXNET_PARAMS
        return segment_table_of(S.walk(S.alexnet(3), 3, 224, 224))[0]
    else:
        raise AssertionError(kind)
    return np.concatenate([[0], np.sort(np.asarray(cuts, np.int64)), [n]]).astype(np.uint32)


def tables_for(n):
    if n < 1023:
        return ["one", "seven"]
    if n == 1023:
        return ["one", "seven", "300", "each"]
    if n == ALEXNET_PARAMS:
        return ["one", "seven", "300", "net"]
    return ["seven", "300"]


def make_flags(pattern, n_seg):
    if pattern == "all":
        return np.full(n_seg, SEG_DECAY | SEG_ADAPT, np.uint32)
    if pattern == "none":  # no trust ratio anywhere; decay on every other segment
        return np.array([SEG_DECAY if s % 2 == 0 else 0 for s in range(n_seg)], np.uint32)
    return np.array([(SEG_DECAY | SEG_ADAPT, SEG_ADAPT, SEG_DECAY, 0)[s % 4] for s in range(n_seg)], np.uint32)


def make_data(n, bounds, seed, steps):
    """parameters and `steps` gradients: every 97th gradient exactly 0; with three or more segments the gradients of segment 1 are all 0
    (its state stays zero) and the parameters of segment 2 start at 0"""
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    grads = [rs.standard_normal(n).astype(np.float32) for _ in range(steps)]
    for g in grads:
        g[::97] = 0.0
        if len(bounds) > 3:
            g[bounds[1]:bounds[2]] = 0.0
    if len(bounds) > 3:
        p[bounds[2]:bounds[3]] = 0.0
    return p, grads


# ---- segment norms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, ALEXNET_PARAMS, BIG])
def test_segment_norms(T, n):
    """every table and both alignments: each norm within one ulp of ref_segment_norms, two runs give identical words, the guard floats
    around the input and the output stay intact"""
    from cnn_amd import capi

    rs = np.random.RandomState(n % 1000)
    x = rs.standard_normal(n).astype(np.float32)
    x[::97] = 0.0
    for kind in tables_for(n):
        bounds = make_table(kind, n, 40 + n % 1000)
        n_seg = len(bounds) - 1
        if n_seg >= 3:
            x[bounds[1]:bounds[2]] = 0.0
        want = ref_segment_norms(x, bounds)
        lw = capi.Layerwise(bounds, np.zeros(n_seg, np.uint32))
        words = []
        for offset in (False, True):
            xb = Buf(T, x, offset)
            for _ in range(2):
                out = Buf(T, np.full(n_seg, -1.0, np.float32), False)
                lw.segment_norms(xb.view, out.view)
                T.cuda.synchronize()
                got = out.get()
                norms_close(got, want, f"n={n} table={kind} offset={offset}")
                words.append(bits(got))
            assert same(xb.get(), x)
        assert all(np.array_equal(words[0], w) for w in words[1:]), f"n={n} table={kind}: the words differ between runs or alignments"
        if n_seg >= 3:
            assert want[1] == 0 and words[0][1] == 0
        lw.close()
    print(f"one-ulp allowance used by {ALLOWANCE_USED['norms']} of {ALLOWANCE_USED['of']} norms so far")


# ---- the update kernels against the reference ----------------------------------------------------------------------------------------
#          grad_scale, previous, weight decay, flags
COMBOS = [(1.0, False, 0.0, "all"), (0.125, True, 1e-2, "mixed"), (1.0, True, 1e-2, "none"), (0.125, False, 1e-2, "all"),
          (1.0, False, 1e-2, "mixed"), (0.125, True, 0.0, "none"), (1.0, True, 0.0, "mixed"), (0.125, False, 0.0, "all")]
LAMB = dict(beta1=0.9, beta2=0.999, eps=1e-6)
LARS = dict(momentum=0.9, trust_coefficient=1e-3, eps=1e-8)


def run_lamb(T, n, kind, offset, combo, seed, steps=(1, 2, 3)):
    from cnn_amd import capi

    scale, with_prev, wd, pattern = combo
    bounds = make_table(kind, n, seed)
    flags = make_flags(pattern, len(bounds) - 1)
    p, grads = make_data(n, bounds, seed + 1, len(steps))
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lw = capi.Layerwise(bounds, flags)
    pb, mb, vb, ub = Buf(T, p, offset), Buf(T, m, offset), Buf(T, v, offset), Buf(T, np.full(n, 7.0, np.float32), offset)
    prevb = Buf(T, np.zeros(n, np.float32), offset) if with_prev else None
    for step, g in zip(steps, grads):
        gb = Buf(T, g, offset)
        lw.lamb_update(pb.view, gb.view, mb.view, vb.view, ub.view, LR, weight_decay=wd, step=step, grad_scale=scale,
                       previous=prevb.view if with_prev else None, **LAMB)
        wn, un, ratio = lw.stats()
        tag = f"lamb n={n} table={kind} offset={offset} combo={combo} step={step}"
        r, _, _ = ref_lamb_moments(p, g, m, v, bounds, flags, step, weight_decay=wd, grad_scale=scale, **LAMB)
        norms_close(wn, ref_segment_norms(p, bounds), tag + " w_norm")
        norms_close(un, ref_segment_norms(r, bounds), tag + " u_norm")
        want_p, want_m, want_v, want_r, want_ratio = ref_lamb_step(p, g, m, v, bounds, flags, step, LR, wn, un, weight_decay=wd, grad_scale=scale,
                                                                   **LAMB)
        assert same(ratio, want_ratio), tag + " ratio"
        if pattern == "none":
            assert np.all(ratio == np.float32(1))
        assert same(ub.get(), want_r), tag + " update"
        assert same(mb.get(), want_m) and same(vb.get(), want_v), tag + " moments"
        assert same(pb.get(), want_p), tag + " params"
        assert same(gb.get(), g), tag + " gradients changed"
        if with_prev:
            assert same(prevb.get(), p), tag + " previous"
        p, m, v = want_p, want_m, want_v
    lw.close()
    return len(flags)


def run_lars(T, n, kind, offset, combo, seed, steps=3, nesterov=False, momentum=None):
    from cnn_amd import capi

    scale, with_prev, wd, pattern = combo
    opts = dict(LARS, momentum=LARS["momentum"] if momentum is None else momentum)
    bounds = make_table(kind, n, seed)
    flags = make_flags(pattern, len(bounds) - 1)
    p, grads = make_data(n, bounds, seed + 1, steps)
    v = np.zeros(n, np.float32)
    lw = capi.Layerwise(bounds, flags)
    pb, vb = Buf(T, p, offset), Buf(T, v, offset)
    prevb = Buf(T, np.zeros(n, np.float32), offset) if with_prev else None
    for step, g in enumerate(grads):
        gb = Buf(T, g, offset)
        lw.lars_update(pb.view, gb.view, vb.view if opts["momentum"] else None, LR, weight_decay=wd, nesterov=nesterov, grad_scale=scale,
                       previous=prevb.view if with_prev else None, **opts)
        wn, un, ratio = lw.stats()
        tag = f"lars n={n} table={kind} offset={offset} combo={combo} step={step}"
        norms_close(wn, ref_segment_norms(p, bounds), tag + " w_norm")
        # (u_norm has grad_scale folded in; 1/8 is a power of two, the product is exact, so the allowance is still one ulp)
        gn = ref_segment_norms(g, bounds)
        norms_close(un, gn * np.float32(scale) if np.float32(scale) != np.float32(1) else gn, tag + " u_norm")
        want_p, want_v, want_gnt, want_ratio = ref_lars_step(p, g, v, bounds, flags, LR, wn, un, weight_decay=wd, nesterov=nesterov,
                                                             grad_scale=scale, norm_is_scaled=True, **opts)
        assert same(un, want_gnt), tag + " u_norm"
        assert same(ratio, want_ratio), tag + " ratio"
        assert same(pb.get(), want_p), tag + " params"
        assert same(vb.get(), want_v), tag + " velocity"
        assert same(gb.get(), g), tag + " gradients changed"
        if with_prev:
            assert same(prevb.get(), p), tag + " previous"
        p, v = want_p, want_v
    lw.close()
    return len(flags)


@pytest.mark.parametrize("optimizer", ["lamb", "lars"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, ALEXNET_PARAMS])
def test_update_kernels_equal_the_reference(T, n, optimizer):
    """every table of this size x both alignments x COMBOS (grad_scale 1 and 1/8, previous null and non-null, weight decay 0 and 1e-2,
    every flag pattern; each pair of those values occurs), three steps so the state carries"""
    seed = 2000 + n % 1000
    seen = set()
    for kind in tables_for(n):
        for offset in (False, True):
            for k, combo in enumerate(COMBOS):
                seed += 1
                if optimizer == "lamb":
                    seen.add(run_lamb(T, n, kind, offset, combo, seed))
                else:
                    seen.add(run_lars(T, n, kind, offset, combo, seed, nesterov=k % 2 == 1, momentum=0.0 if k == 4 else None))
    if n >= 1023:
        assert 300 in seen and 7 in seen and 1 in seen
    if n == 1023:
        assert 1023 in seen
    print(f"one-ulp allowance used by {ALLOWANCE_USED['norms']} of {ALLOWANCE_USED['of']} norms so far")


def test_lamb_at_step_1000(T):
    """the bias corrections far from step 1 (bc1 = 1 - 0.9^1000 rounds to 1, bc2s = sqrt(1 - 0.999^1000) ~ 0.795)"""
    run_lamb(T, 1023, "300", False, COMBOS[1], 77, steps=(1000, 1001))
    run_lamb(T, ALEXNET_PARAMS, "net", True, COMBOS[4], 78, steps=(1000,))


@pytest.mark.parametrize("optimizer,offset,kind", [("lamb", False, "300"), ("lars", True, "seven")])
def test_update_kernels_beyond_2_pow_24(T, optimizer, offset, kind):
    """n = 2^24 + 5: 16385 chunks, element indices fp32 could not hold, a last chunk of 5 elements"""
    if optimizer == "lamb":
        run_lamb(T, BIG, kind, offset, COMBOS[1], 91, steps=(1, 2))
    else:
        run_lars(T, BIG, kind, offset, COMBOS[4], 92, steps=2, nesterov=True)


@pytest.mark.parametrize("n", [5, 1023, ALEXNET_PARAMS])
def test_lars_without_adapt_is_momentum_sgd_on_the_device(T, n):
    """no ADAPT flag: cnn_lars_update equals cnn_sgd_momentum_update with the DECAY segments as its range table, bit for bit --
    parameters, velocity and `previous`, three steps"""
    from cnn_amd import capi

    for kind in tables_for(n):
        for offset in (False, True):
            for momentum, wd, nesterov, scale in [(0.9, 5e-4, False, 1.0), (0.9, 5e-4, True, 0.125), (0.0, 1e-2, False, 1.0), (0.9, 0.0, False, 0.125)]:
                bounds = make_table(kind, n, 300 + n % 1000)
                flags = make_flags("none", len(bounds) - 1)
                ranges = [(int(bounds[s]), int(bounds[s + 1])) for s in range(len(flags)) if flags[s] & SEG_DECAY]
                p, grads = make_data(n, bounds, 301, 3)
                lw = capi.Layerwise(bounds, flags)
                bufs = [[Buf(T, p, offset), Buf(T, np.zeros(n, np.float32), offset), Buf(T, np.zeros(n, np.float32), offset)] for _ in range(2)]
                for g in grads:
                    gb = Buf(T, g, offset)
                    (pa, va, ka), (pb, vb, kb) = bufs
                    lw.lars_update(pa.view, gb.view, va.view if momentum else None, LR, momentum, wd, 1e-3, 1e-8, nesterov, scale, ka.view)
                    capi.sgd_momentum_update(pb.view, gb.view, vb.view, LR, momentum, wd, nesterov, scale, ranges, kb.view)
                    T.cuda.synchronize()
                    tag = f"n={n} table={kind} offset={offset} opt={(momentum, wd, nesterov, scale)}"
                    assert same(pa.get(), pb.get()) and same(va.get(), vb.get()) and same(ka.get(), kb.get()), tag
                    assert np.all(lw.stats()[2] == np.float32(1))
                assert not same(bufs[0][0].get(), p)
                lw.close()


def test_launches_per_call_do_not_depend_on_the_number_of_segments(T):
    """the library's launch log: three launches per update call (the pass that produces the partial sums, the finish, the step), two
    per cnn_segment_norms, for 1, 40 and 300 segments and for both alignments"""
    from cnn_amd import capi

    n = ALEXNET_PARAMS
    host = np.random.RandomState(9).standard_normal(n).astype(np.float32)
    for offset in (False, True):
        for n_seg in (1, 40, 300):
            cuts = np.sort(np.random.RandomState(n_seg).choice(np.arange(1, n), n_seg - 1, replace=False))
            bounds = np.concatenate([[0], cuts, [n]]).astype(np.uint32)
            lw = capi.Layerwise(bounds, make_flags("mixed", n_seg))
            p, g, m, v, u, prev = (Buf(T, host, offset) for _ in range(6))
            out = Buf(T, np.zeros(n_seg, np.float32), False)
            calls = {
                "lamb": (lambda: lw.lamb_update(p.view, g.view, m.view, v.view, u.view, LR, weight_decay=1e-2, previous=prev.view),
                         ["lamb_apply", "lamb_moments", "seg_finish"]),
                "lars": (lambda: lw.lars_update(p.view, g.view, v.view, LR, 0.9, 5e-4, previous=prev.view), ["lars_apply", "lars_norms", "seg_finish"]),
                "norms": (lambda: lw.segment_norms(g.view, out.view), ["seg_finish", "seg_norm_partial"]),
            }
            for name, (call, kernels) in calls.items():
                T.cuda.synchronize()
                capi.kernel_timing(1)
                call()
                rep = capi.kernel_timing_report()
                capi.kernel_timing(0)
                got = sorted((k.split("|")[0], cnt) for k, (cnt, _) in rep.items())
                assert got == [(k, 1) for k in kernels], (name, offset, n_seg, rep)
                assert len(got) <= 4
                assert all(("scalar" in k) == offset for k in rep if not k.startswith("seg_finish")), rep
            lw.close()


def test_bad_arguments_write_nothing(T):
    from cnn_amd import capi

    lib = capi.load()
    n = 1023
    for bounds, flags in [([0, 10, 10, n], [0, 0, 0]), ([0, 500, 400, n], [0, 0, 0]), ([0], [])]:  # empty, unsorted, none
        with pytest.raises(capi.CnnAmdError, match="cnn_layerwise_create"):
            capi.Layerwise(bounds, flags)
    host = np.random.RandomState(1).standard_normal(n).astype(np.float32)
    lw = capi.Layerwise([0, 100, n], [3, 3])
    p, g, m, v, u, prev = (Buf(T, host, False) for _ in range(6))
    short = Buf(T, host[:n - 1], False)  # the table's last bound is not this tensor's n
    with pytest.raises(capi.CnnAmdError, match="n=1023"):
        lw.lamb_update(short.view, g.view, m.view, v.view, u.view, LR)
    with pytest.raises(capi.CnnAmdError, match="n=1023"):
        lw.lars_update(p.view, short.view, v.view, LR, 0.9)
    with pytest.raises(capi.CnnAmdError, match="n=1023"):
        lw.segment_norms(short.view)
    for bad in (dict(step=0), dict(eps=0.0), dict(beta1=1.0), dict(beta2=1.0), dict(weight_decay=-1.0)):
        with pytest.raises(capi.CnnAmdError, match="cnn_lamb_update"):
            lw.lamb_update(p.view, g.view, m.view, v.view, u.view, LR, previous=prev.view, **bad)
    for bad in (dict(eps=0.0), dict(trust_coefficient=0.0), dict(momentum=-0.5), dict(weight_decay=-1.0)):
        with pytest.raises(capi.CnnAmdError, match="cnn_lars_update"):
            lw.lars_update(p.view, g.view, v.view, LR, **{"momentum": 0.9, **bad}, previous=prev.view)
    with pytest.raises(capi.CnnAmdError, match="null velocity"):
        lw.lars_update(p.view, g.view, None, LR, 0.9)
    opt = capi.LambOptions(LR, 0.9, 0.999, 1e-6, 0.0, 1)
    assert lib.cnn_lamb_update(lw.h, capi._ptr(p.view), capi._ptr(g.view), None, capi._ptr(v.view), capi._ptr(u.view), C.byref(opt), 1.0, None,
                               capi._stream()) != 0
    assert lib.cnn_lamb_update(None, capi._ptr(p.view), capi._ptr(g.view), capi._ptr(m.view), capi._ptr(v.view), capi._ptr(u.view), C.byref(opt),
                               1.0, None, capi._stream()) != 0
    T.cuda.synchronize()
    for b in (p, g, m, v, u, prev):
        assert same(b.get(), host)
    assert not np.any(np.concatenate(lw.stats()))  # (zeroed at creation, never written)
    lw.close()


# ---- whole nets ------------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "lamb": ("lamb", dict(weight_decay=1e-2)),
    "lars": ("lars", dict(momentum=0.9, weight_decay=5e-4)),
    "lamb_bias_and_norm": ("lamb", dict(weight_decay=1e-2, decay_bias_and_norm=True, adapt_bias_and_norm=True)),
    "lars_bias_and_norm": ("lars", dict(momentum=0.9, weight_decay=5e-4, decay_bias_and_norm=True, adapt_bias_and_norm=True)),
}


def arm(net, variant):
    kind, kw = VARIANTS[variant]
    (net.set_lamb if kind == "lamb" else net.set_lars)(**kw)
    return kind, kw


def table_of(layout, kw):
    return segment_table_of(layout, kw.get("decay_bias_and_norm", False), kw.get("adapt_bias_and_norm", False))


def host_step(kind, kw, bounds, flags, p, g, state, step, stats, tag):
    """one reference step from the device's statistics -> (p', state'); the norms are held to the fp64 values within the allowance and
    the ratios to the reference bit for bit on the way"""
    wn, un, ratio = stats
    norms_close(wn, ref_segment_norms(p, bounds), tag + " w_norm")
    if kind == "lamb":
        r, _, _ = ref_lamb_moments(p, g, state[0], state[1], bounds, flags, step, eps=1e-6, weight_decay=kw["weight_decay"])
        norms_close(un, ref_segment_norms(r, bounds), tag + " u_norm")
        p_new, m, v, _, want_ratio = ref_lamb_step(p, g, state[0], state[1], bounds, flags, step, LR, wn, un, eps=1e-6, weight_decay=kw["weight_decay"])
        assert same(ratio, want_ratio), tag + " ratio"
        return p_new, [m, v]
    norms_close(un, ref_segment_norms(g, bounds), tag + " g_norm")
    p_new, v, _, want_ratio = ref_lars_step(p, g, state[0], bounds, flags, LR, wn, un, kw["momentum"], kw["weight_decay"])
    assert same(ratio, want_ratio), tag + " ratio"
    return p_new, [v]


def get_state(net, kind):
    if kind == "lamb":
        m, v, t = net.get_adam_state()
        return [m, v], t
    return [net.get_velocity()], None


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("which", ["alexnet", "alexnet_bn", "small_bn"])
def test_train_step_equals_host_stepped_net(T, which, variant):
    """net A: three train_steps under set_lamb / set_lars; net B: the plain sequence (forward_backward), the gradient arena comes back
    and the reference steps on the host with A's device norms (trust_stats) of that step.  Parameters, state and last_loss() agree
    bit for bit at every step, BatchNorm2D's moving statistics are what the forward passes alone produce, the net's segment table is
    the one computed here from the layout"""
    layout, p0, x, labels = net_inputs(T, which, 500)
    moving = moving_stat_mask(layout)
    a, b = make_net(which), make_net(which)
    a.set_params(p0)
    b.set_params(p0)
    assert a.segment_count() == 0 and not a.layerwise_active()
    kind, kw = arm(a, variant)
    bounds, flags = table_of(layout, kw)
    got_bounds, got_flags = a.segment_table()
    assert a.layerwise_active() and a.segment_count() == len(flags)
    assert np.array_equal(got_bounds, bounds) and np.array_equal(got_flags, flags)
    assert int(bounds[-1]) == p0.size and not np.any(np.repeat(flags, np.diff(bounds.astype(np.int64)))[moving])
    state = [np.zeros(p0.size, np.float32) for _ in range(2 if kind == "lamb" else 1)]
    for step in range(1, 4):
        b.forward_backward(x, labels)
        loss, g, p = b.last_loss(), b.get_grads(), b.get_params()
        assert not np.any(g[moving])
        a.train_step(x, labels, LR)
        p_new, state = host_step(kind, kw, bounds, flags, p, g, state, step, a.trust_stats(), f"{which} {variant} step {step}")
        got_state, got_t = get_state(a, kind)
        got_p = a.get_params()
        print(f"{which} {variant} step {step}: loss {a.last_loss()!r} / {loss!r}, params differ at {int((bits(got_p) != bits(p_new)).sum())} of {p.size}")
        assert a.last_loss() == loss, step
        assert same(got_p, p_new), f"step {step}: parameters"
        assert all(same(x_, y_) for x_, y_ in zip(got_state, state)), f"step {step}: state"
        assert got_t in (None, step)
        assert same(p_new[moving], p[moving]) and same(got_p[moving], p[moving]), f"step {step}: moving statistics"
        assert all(not np.any(s[moving]) for s in state)
        b.set_params(p_new)
    assert not same(a.get_params(), p0)
    a.close()
    b.close()
    print(f"one-ulp allowance used by {ALLOWANCE_USED['norms']} of {ALLOWANCE_USED['of']} norms so far")


@pytest.mark.parametrize("variant", ["lamb", "lars"])
def test_the_clip_runs_in_front_of_the_layerwise_step(T, variant):
    """set_grad_clip(half of step 1's norm): the reference is ref_clip (from A's device norm), then the step"""
    which = "alexnet"
    layout, p0, x, labels = net_inputs(T, which, 510)
    a, b = make_net(which), make_net(which)
    a.set_params(p0)
    b.set_params(p0)
    kind, kw = arm(a, variant)
    bounds, flags = table_of(layout, kw)
    state = [np.zeros(p0.size, np.float32) for _ in range(2 if kind == "lamb" else 1)]
    max_norm = None
    for step in range(1, 4):
        b.forward_backward(x, labels)
        g, p = b.get_grads(), b.get_params()
        if max_norm is None:
            max_norm = 0.5 * float(ref_total_norm(g))
            a.set_grad_clip(max_norm)
        a.train_step(x, labels, LR)
        norm, coef = a.last_grad_norm()
        assert ulps(norm, ref_total_norm(g)) <= 1
        g_clipped, want_coef = ref_clip(g, norm, max_norm)
        assert bits(np.asarray([coef]))[0] == bits(np.asarray([want_coef]))[0] and (step > 1 or coef < 1)
        p_new, state = host_step(kind, kw, bounds, flags, p, g_clipped, state, step, a.trust_stats(), f"clip {variant} step {step}")
        assert a.last_loss() == b.last_loss() and same(a.get_params(), p_new), f"{variant} step {step}"
        b.set_params(p_new)
    a.close()
    b.close()


@pytest.mark.parametrize("variant", ["lamb_bias_and_norm", "lars"])
@pytest.mark.parametrize("which", ["alexnet", "alexnet_bn"])
def test_forced_one_rank_exchange(T, which, variant, lib_option):
    """the data-parallel route (all-reduce, then the layer-wise step with grad_scale 1 / world) forced on with ONE rank
    (DP_FORCE_EXCHANGE: every sum is an identity): losses, parameters, state and statistics of three steps equal the
    no-communicator run's"""
    from cnn_amd.dp import RcclComm

    layout, p0, x, labels = net_inputs(T, which, 520)
    comm = RcclComm(None, 1, 0)
    outs = []
    for use_comm in (False, True):
        net = make_net(which)
        net.set_params(p0)
        kind, _ = arm(net, variant)
        if use_comm:
            net.set_comm(comm.handle, 1)
            lib_option("DP_FORCE_EXCHANGE", "1")
        losses = []
        for _ in range(3):
            net.train_step(x, labels, LR)
            losses.append(net.last_loss())
        outs.append((losses, net.get_params(), get_state(net, kind)[0], net.trust_stats()))
        net.close()
        lib_option("DP_FORCE_EXCHANGE", None)
    comm.destroy()
    assert outs[0][0] == outs[1][0] and same(outs[0][1], outs[1][1])
    assert all(same(x_, y_) for x_, y_ in zip(outs[0][2], outs[1][2])) and all(same(x_, y_) for x_, y_ in zip(outs[0][3], outs[1][3]))


@pytest.mark.parametrize("variant", ["lamb_bias_and_norm", "lars_bias_and_norm"])
def test_state_round_trip(T, tmp_path, variant):
    """weights + optimizer state saved after step 2 and loaded into a fresh net: the file's optimizer becomes active and step 3 is the
    uninterrupted run's, bit for bit; a file for another n_params is status 3, a truncated one status 2, and neither changes anything"""
    which = "alexnet_bn"
    layout, p0, x, labels = net_inputs(T, which, 530)
    a = make_net(which)
    a.set_params(p0)
    kind, kw = arm(a, variant)
    for _ in range(2):
        a.train_step(x, labels, LR)
    model, state = str(tmp_path / "step2.model"), str(tmp_path / "step2.state")
    a.save_checkpoint(model)
    a.save_optimizer_state(state)
    magic, arenas = (b"CNNALMB1", 2) if kind == "lamb" else (b"CNNALRS1", 1)
    assert open(state, "rb").read(8) == magic and os.path.getsize(state) == 48 + arenas * 4 * a.n_params
    a.train_step(x, labels, LR)
    want = (a.last_loss(), a.get_params(), get_state(a, kind), a.trust_stats(), a.segment_table())
    a.close()
    b = make_net(which)
    b.load_checkpoint(model)
    assert not b.layerwise_active()
    b.load_optimizer_state(state)
    assert b.layerwise_active() and all(np.array_equal(x_, y_) for x_, y_ in zip(b.segment_table(), want[4]))
    b.train_step(x, labels, LR)
    got = (b.last_loss(), b.get_params(), get_state(b, kind), b.trust_stats())
    assert got[0] == want[0] and same(got[1], want[1]) and got[2][1] == want[2][1]
    assert all(same(x_, y_) for x_, y_ in zip(got[2][0], want[2][0])) and all(same(x_, y_) for x_, y_ in zip(got[3], want[3]))
    again = str(tmp_path / "again.state")
    b.save_optimizer_state(again)
    assert open(again, "rb").read(48)[:8] == magic
    other = make_net("small_bn")
    assert other.n_params != b.n_params
    assert other.lib.cnnh_net_load_optimizer_state(other.h, state.encode()) == 3
    assert not other.layerwise_active() and other.segment_count() == 0 and other.adam_ptrs() == (None, None) and not other.velocity_ptr()
    other.close()
    truncated = str(tmp_path / "short.state")
    open(truncated, "wb").write(open(state, "rb").read()[:-8])
    before = get_state(b, kind)
    assert b.lib.cnnh_net_load_optimizer_state(b.h, truncated.encode()) == 2
    after = get_state(b, kind)
    assert all(same(x_, y_) for x_, y_ in zip(before[0], after[0])) and before[1] == after[1]
    b.close()


def test_switching_keeps_the_state_and_the_last_one_set_is_active(T):
    """set_adam -> set_lamb shares the moments and the step counter, set_optimizer -> set_lars the velocity; the launch log shows the
    kernels of the optimizer set last, three launches per layer-wise step and no other step kernel"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 540)
    net = make_net("alexnet")
    net.set_params(p0)
    net.set_adam()
    net.train_step(x, labels, LR)
    m1, v1, t1 = net.get_adam_state()
    net.set_lamb(weight_decay=1e-2)
    m, v, t = net.get_adam_state()
    assert t1 == t == 1 and same(m, m1) and same(v, v1) and np.any(m1)
    log = step_kernels(T, net, x, labels, steps=2)
    assert {k.split("|")[0]: c for k, c in log.items() if k.startswith(("lamb_", "seg_", "lars_", "adam_", "sgd", "clip_"))} == \
        {"lamb_moments": 2, "seg_finish": 2, "lamb_apply": 2}, log
    assert net.get_adam_state()[2] == 3
    net.set_lars(0.9, 5e-4)
    assert not np.any(net.get_velocity())
    log = step_kernels(T, net, x, labels, steps=2)
    assert {k.split("|")[0]: c for k, c in log.items() if k.startswith(("lamb_", "seg_", "lars_", "adam_", "sgd", "clip_"))} == \
        {"lars_norms": 2, "seg_finish": 2, "lars_apply": 2}, log
    vel = net.get_velocity()
    assert np.any(vel) and net.get_adam_state()[2] == 3
    net.set_optimizer(0.9, 5e-4)
    assert not net.layerwise_active() and same(net.get_velocity(), vel)
    log = step_kernels(T, net, x, labels, steps=1)
    assert any(k.startswith("sgdm_vec|") for k in log) and not any(k.startswith(("lamb_", "lars_", "seg_")) for k in log)
    net.set_adam()
    log = step_kernels(T, net, x, labels, steps=1)
    assert any(k.startswith("adam_vec|") for k in log) and not any(k.startswith(("lamb_", "lars_", "seg_", "sgdm")) for k in log)
    assert net.get_adam_state()[2] == 4
    net.close()


def test_plain_step_after_lamb_is_the_default_path(T, golden_dir):
    """set_lamb / set_lars, then set_optimizer(0, 0): three train_steps of the reference net launch exactly the kernels of the commit
    before the optimizers (tests/golden/train_step_kernels_before_optimizer.json, at that test's inputs) and end with the parameters
    of a net that never had an optimizer"""
    layout, p0, x, labels = net_inputs(T, "alexnet", 340)
    golden = json.load(open(os.path.join(golden_dir, "train_step_kernels_before_optimizer.json")))
    runs = {}
    for mode in ("never", "lamb_then_plain"):
        net = make_net("alexnet")
        net.set_params(p0)
        if mode != "never":
            net.set_lamb(weight_decay=1e-2)
            net.set_lars(0.9, 5e-4)
            net.set_optimizer(0, 0)
            assert not net.layerwise_active()
        runs[mode] = (step_kernels(T, net, x, labels), net.get_params())
        net.close()
    assert runs["never"][0] == golden
    assert runs["lamb_then_plain"][0] == golden, sorted(set(runs["lamb_then_plain"][0].items()) ^ set(golden.items()))
    assert same(runs["never"][1], runs["lamb_then_plain"][1])
