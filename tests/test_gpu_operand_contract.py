"""Nothing outside an input tensor may reach a result: every read-only operand of the C ABI between poison (tests/guarded.operand).

tests/test_gpu_scratch_contract.py holds the SCRATCH of every call to its size contract; the operands -- x, w, bias, dy, relu_below, pool
masks, labels, gradients, optimizer arenas -- were uploaded with a plain .cuda(), so their neighbours in memory were whatever the caching
allocator last held: finite, small, often zero.  Several kernels read past a row, a plane or a tensor on purpose and repair it afterwards
(16-byte DMA units over ragged rows, zeros in LDS instead of masks, rows staged past a plane's end and selected away, 16-byte / scalar
switches at heads and tails); one that lets such a value into a sum passes every other test.  Here every operand of every call is the
interior of a guarded allocation filled with quiet NaNs or with the bytes 0x5A (1.5e16 as a float), at the allocation's natural alignment
and shifted by 4 (8, 12) bytes so that 16-byte units straddle the tensor's first and last element.  Scratch and outputs stay guarded as in
the sibling module, so both contracts are tested together.

The dead elements of a convolution input (tests/conv_unread.py: positions no window covers -- the last row and column of 224 x 224 at
k 3 s 2, the odd lattice of a 1x1 stride-2 layer) carry the same poison INSIDE x and relu_below; tests/test_conv_unread.py proves on the
CPU that the oracle's results do not depend on them and that its dx is +0.0 there.

What is asserted: the sibling's criteria (the CPU oracle at REL_TOL through tests.util.assert_close, the compositions bit for bit) -- a NaN
or 1.5e16 in one addend misses them by orders of magnitude; the digests of tests/golden/conv_routes.json; +0.0 in dx at dead positions;
every canary of every operand, scratch buffer and output (a store through an input pointer).  No tolerance of its own.

An over-read that stays inside the guard zone and reaches no result is not flagged: whether it could cross the end of a real allocation
cannot be tested without risking a fault.  A HIP error ends the session (pytest.exit(returncode=3)) as in the sibling module."""
import hashlib

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import conv_route_cases as R
from tests import guarded
from tests.conv_unread import poisoned, unread_mask
from tests.test_gpu_scratch_contract import (MUST_LAUNCH, PARAMS, Refused, Run, T, _check_conv_results, _id, _plain_calls, _pool_family,  # noqa: F401
                                             _prepared_calls, _same, bits, dev, golden, host)
from tests.util import normal_scaled, uniform01, uniform_pm1

pytestmark = pytest.mark.gpu

PLACEMENTS = ((guarded.NAN, 0), (guarded.BYTES, 0), (guarded.BYTES, 4))  # (poison, shift in bytes): the conv entry points ask for 4-byte alignment
WORD = {guarded.NAN: 0x7FC00000, guarded.BYTES: 0x5A5A5A5A}
POOL_CALLS = ("prepare_filters", "relu_maxpool2_forward", "relu_maxpool2_forward_prepared", "backward_weight_pooled2", "backward_data_pooled2",
              "backward_data_pooled2_prepared", "backward_weight_pooled2_sgd", "backward_weight_pooled2_sgd_keep")


class Place:
    """every operand of one run: place(name, array) -> the array between `poison`, `shift` bytes off the 256-byte boundary"""

    def __init__(self, poison, shift, note=""):
        self.poison, self.shift, self.guards = poison, shift, []
        self.label = f"operands in {poison} + {shift} bytes{note}"

    def __call__(self, name, array):
        return guarded.operand(array, self.poison, self.guards, name, self.shift)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _conv_run(T, case, place, data, ref, may_refuse, problems):
    """every call of the sibling test (without its short buffers) with the operands placed by `place` -> the Run"""
    from cnn_amd import capi

    B, Ci, H, W, Co, k, s, pad = case[:8]
    r = Run(T, case, place.poison, data, problems, place=place)
    for name, fn in _plain_calls(r).items():
        r.call(name, fn)
    for g in (r.pf, r.pd):
        g.refill()
    prepared = r.call("prepare_filters", lambda keep: capi.prepare_filters([r.conv], [r.w], [r.b], [r.pf.view], [r.pd.view]) or {})
    expected = list(_plain_calls(r)) + ["prepare_filters"] + list(_prepared_calls(r))
    if prepared is not None:
        for name, fn in _prepared_calls(r).items():
            r.call(name, fn)
    _check_conv_results(r, ref, may_refuse)
    if r.conv.relu_maxpool2_supported():
        _pool_family(r, packed=False)
        expected += ["pool/" + c for c in POOL_CALLS]
        if capi.Conv2d(B, Ci, H, W, Co, k, s, pad).pool_mask_packed_supported():
            _pool_family(r, packed=True)
            expected += ["pool/packed/" + c for c in POOL_CALLS + ("pool_mask_unpack",)]
        for call, outs in r.results.items():
            if call.startswith("pool/") and isinstance(outs, Refused) and not may_refuse(call):
                problems.append(f"{call} [{r.where}]: refused with full-size buffers: {outs}")
    # refusals must not shrink the test: every call that may not refuse (the calls that run in the sibling test) has run and left results
    for call in expected:
        if not may_refuse(call) and not isinstance(r.results.get(call), dict):
            problems.append(f"{call} [{r.where}]: did not run ({r.results.get(call)!r})")
    return r


@pytest.mark.parametrize("param", PARAMS, ids=_id)
def test_conv_calls_read_nothing_outside_their_operands(T, param, golden, lib_option):
    from cnn_amd import capi

    case, opts = param
    for name, value in opts:
        lib_option(name, value)
    B, Ci, H, W, Co, k, s, pad = case[:8]
    layer_data = not opts and case in R.HAND_PICKED  # (tests/conv_route_cases._Layer's seeds: the data the digests were recorded with)
    seed = 9000 + 10 * R.HAND_PICKED.index(case) if layer_data else 9000 + 7 * PARAMS.index(param)
    x, w, b = uniform01(seed, (B, Ci, H, W)), normal_scaled(seed + 1, (Co, Ci, k, k)), normal_scaled(seed + 2, (Co,))
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    dy = uniform_pm1(seed + 3, (B, Co, Ho, Wo))
    relu_below = np.maximum(x - np.float32(0.5), np.float32(0))
    dead = unread_mask(case)
    has_dead = bool(dead.any())
    x0, relu0 = x.copy(), relu_below.copy()
    x0[:, :, dead] = 0
    relu0[:, :, dead] = 0
    # the reference never sees a poison: the oracle on zeros at the dead positions (tests/test_conv_unread.py: it does not read them)
    xp = np.pad(x0, ((0, 0), (0, 0), (pad, pad), (pad, pad))) if pad else x0
    y_ref = O.conv2d_forward(xp, w, b, s)
    gw_ref, gb_ref, dxp = O.conv2d_backward(xp, dy, w, s)
    dx_ref = dxp[:, :, pad:pad + H, pad:pad + W] if pad else dxp
    ref = (y_ref, gw_ref, gb_ref, dx_ref, np.where(relu0 <= 0, np.float32(0), dx_ref))

    recorded = golden.get(R.key(case), {})
    pinned = recorded if not opts else {}
    flagged = len(case) > 8 and case[8] != 0
    may_refuse = lambda call: ("rc" in recorded.get(call, {}) or  # (the sibling test's rule, unchanged)
                               (flagged and "backward" in call and "backward_data" not in call and not call.startswith("pool/")))
    problems, runs = [], []
    T.cuda.synchronize()
    capi.kernel_timing(1)
    try:
        for poison, shift in PLACEMENTS:
            data = (poisoned(x, dead, WORD[poison]), w, b, dy, poisoned(relu_below, dead, WORD[poison])) if has_dead else (x, w, b, dy, relu_below)
            runs.append(_conv_run(T, case, Place(poison, shift), data, ref, may_refuse, problems))
        zeros = _conv_run(T, case, Place(guarded.NAN, 0, ", zeros at the dead positions"), (x0, w, b, dy, relu0), ref, may_refuse, problems) if has_dead else None
        T.cuda.synchronize()
    finally:
        capi.kernel_timing(0)
    for r in runs:
        for call, kernel in MUST_LAUNCH.get(param, {}).items():
            if kernel not in r.logs.get(call, ()):
                problems.append(f"{call} [{r.where}]: no {kernel} launch, the log holds {sorted(r.logs.get(call, ()))}")
        # the gradient of a dead element is +0.0, bit for bit, in every dx of every call
        for call, outs in r.results.items():
            if has_dead and isinstance(outs, dict) and "dx" in outs and np.any(bits(outs["dx"][:, :, dead]) != 0):
                problems.append(f"{call} [{r.where}]: dx is not +0.0 at {int(np.count_nonzero(np.ascontiguousarray(outs['dx'][:, :, dead]).view(np.uint32)))} dead position(s)")
    # the calls whose digests the route golden pins (they repeat): the same bits under both poisons at shift 0, the pinned digest itself
    # where the data is the recorded one, the bits of a run with zeros at the dead positions otherwise.  (The shifted run: the oracle only.)
    a, b2 = runs[0].results, runs[1].results
    for call, rec in pinned.items():
        if "sha" not in rec or not isinstance(a.get(call), dict) or not isinstance(b2.get(call), dict):
            continue
        for what in a[call]:
            _same(problems, f"{call} {what}: {runs[0].where} vs {runs[1].where}", a[call][what], b2[call][what])
            if zeros is not None and isinstance(zeros.results.get(call), dict):
                _same(problems, f"{call} {what}: {runs[0].where} vs zeros at the dead positions", a[call][what], zeros.results[call][what])
            if layer_data and not has_dead and what in rec["sha"] and _sha(a[call][what]) != rec["sha"][what]:
                problems.append(f"{call} {what} [{runs[0].where}]: not the digest of tests/golden/conv_routes.json")
    assert not problems, f"desc {case} {dict(opts)}: {len(problems)} problem(s)\n  " + "\n  ".join(problems[:40])


# ---- the other loop nests --------------------------------------------------------------------------------------------------------------
class Ops:
    """the operands and outputs of one call under one placement; every tensor (outputs too: the 16-byte / scalar switch looks at all
    pointers) sits `shift` bytes off the 256-byte boundary"""

    def __init__(self, poison, shift):
        self.poison, self.shift, self.guards = poison, shift, []
        self.label = f"{poison} + {shift} bytes"

    def put(self, name, array):
        return guarded.operand(array, self.poison, self.guards, name, self.shift)

    def out(self, name, shape, dtype=None):
        return guarded.output(shape, self.poison, self.guards, name, dtype, self.shift)

    def done(self, T, problems, tag):
        """synchronise (a failure ends the session) and ask every canary"""
        try:
            T.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error behind {tag} [{self.label}]: {e}", returncode=3)
        problems.extend(f"{tag} [{self.label}]: {m}" for m in guarded.check(self.guards))


def _checked(fn, *args):
    """a library call through cnn_amd.capi: a HIP status ends the session, any other status is the test's failure"""
    from cnn_amd import capi
    from tests.test_gpu_scratch_contract import _stop_on_device_error

    try:
        return fn(*args)
    except capi.CnnAmdError as e:
        _stop_on_device_error(e)
        raise


def _bits_same(problems, tag, got, want):
    got, want = np.ascontiguousarray(host(got) if hasattr(got, "detach") else got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(bits(got), bits(want)):
        n = int(np.count_nonzero(got != want)) if got.shape == want.shape else -1
        problems.append(f"{tag}: not bit-identical ({n} element(s) differ)")


THREE = PLACEMENTS
FLAT_N = (1, 2, 3, 5, 64, 67, 1021, 4099)
FLAT_PLACEMENTS = tuple((p, s) for p in guarded.POISONS for s in (0, 4, 8, 12))


def _report(problems, what):
    assert not problems, f"{what}: {len(problems)} problem(s)\n  " + "\n  ".join(problems[:40])


@pytest.mark.parametrize("shape,k,step", [((2, 3, 9, 11), 2, 2), ((1, 5, 7, 7), 3, 2), ((2, 2, 6, 10), 3, 1), ((3, 4, 13, 13), 2, 2)])
def test_maxpool_reads_nothing_outside_its_operands(T, shape, k, step):
    """forward, backward and backward_relu bit for bit as in test_maxpool_bit_exact / test_maxpool_backward_relu_fusion_is_bit_identical
    (ties, signed zeros, NaNs in x); the positions of x no window covers carry the poison and get a gradient of exactly +0.0"""
    from cnn_amd import capi

    B, Cc, H, W = shape
    dead = unread_mask((B, Cc, H, W, Cc, k, step, 0))
    assert dead.any() == (shape == (2, 3, 9, 11) or shape == (3, 4, 13, 13))
    x = uniform_pm1(5, shape)
    flat, rs = x.reshape(-1), np.random.RandomState(1)
    flat[rs.choice(flat.size, flat.size // 6, replace=False)] = 0.5
    flat[rs.choice(flat.size, flat.size // 20, replace=False)] = -0.0
    flat[rs.choice(flat.size, flat.size // 20, replace=False)] = 0.0
    flat[rs.choice(flat.size, max(flat.size // 50, 1), replace=False)] = np.nan
    x0 = x.copy()
    x0[:, :, dead] = 0
    y_ref, m_ref = O.maxpool_forward(x0, k, step)  # (the reference never sees the poison)
    dy = uniform_pm1(6, y_ref.shape)
    dx_ref = O.maxpool_backward(dy, m_ref, shape, k, step)
    # backward_relu: the pool's input is a ReLU layer's output (zeros, ties); the composition of test_maxpool_backward_relu_fusion_is_bit_identical
    # from the oracle's pieces: MaxPool2D::backward, then ReLU::backward (relu.cpp:37-39) with that output
    xr = O.relu_forward(x0)
    assert not np.isnan(xr).any() and (xr == 0).sum() > xr.size // 4
    yr_ref, mr_ref = O.maxpool_forward(xr, k, step)
    dxr_ref = O.relu_backward(xr, O.maxpool_backward(dy, mr_ref, shape, k, step))
    problems = []
    for poison, shift in THREE:
        ops = Ops(poison, shift)
        xd = ops.put("x", poisoned(x, dead, WORD[poison]))
        y, m = ops.out("y", y_ref.shape), ops.out("mask", y_ref.shape, T.int32)
        L = capi.load()
        _checked(capi.check, L.cnn_maxpool2d_forward(capi._ptr(xd), capi._ptr(y), capi._ptr(m), B, Cc, H, W, k, step, capi._stream()), "cnn_maxpool2d_forward")
        y2 = ops.out("y (no mask)", y_ref.shape)
        _checked(capi.check, L.cnn_maxpool2d_forward(capi._ptr(xd), capi._ptr(y2), None, B, Cc, H, W, k, step, capi._stream()), "cnn_maxpool2d_forward")
        ops.done(T, problems, "forward")
        tag = f"[{ops.label}]"
        _bits_same(problems, f"pooled {tag}", y, y_ref)
        _bits_same(problems, f"pooled without a mask {tag}", y2, y_ref)
        _bits_same(problems, f"argmax mask {tag}", m, m_ref)
        dyd, md, mrd, pd = ops.put("dy", dy), ops.put("mask (operand)", m_ref), ops.put("mask behind a ReLU", mr_ref), ops.put("pooled", yr_ref)
        dx, dxr = ops.out("dx", shape), ops.out("dx (relu)", shape)
        _checked(capi.maxpool_backward, dyd, md, shape, k, step, dx)
        _checked(capi.maxpool_backward_relu, dyd, mrd, pd, shape, k, step, dxr)
        ops.done(T, problems, "backward")
        for name, got, want in (("dx", dx, dx_ref), ("dx of backward_relu", dxr, dxr_ref)):
            _bits_same(problems, f"{name} {tag}", got, want)
            if np.any(bits(host(got)[:, :, dead]) != 0):
                problems.append(f"{name} {tag}: not +0.0 at a dead position")
    _report(problems, f"MaxPool2D {shape} k {k} step {step}")


def _flat_data(n, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("n", FLAT_N)
def test_relu_reads_nothing_outside_its_operands(T, n):
    from cnn_amd import capi

    x = uniform_pm1(8, (n,))
    x[::7], x[1::11], x[2::13], x[3::17] = -0.0, 0.0, np.nan, -np.inf  # (test_relu_bit_exact's values)
    d = uniform_pm1(9, (n,))
    y_ref = O.relu_forward(x)
    d_ref = O.relu_backward(y_ref, d)
    problems = []
    for poison, shift in FLAT_PLACEMENTS:
        ops = Ops(poison, shift)
        xd, y = ops.put("x", x), ops.out("y", (n,))
        _checked(capi.relu_forward, xd, y)
        yd, dd = ops.put("y (operand)", y_ref), ops.put("dy (in-out)", d)
        _checked(capi.relu_backward, yd, dd)
        ops.done(T, problems, "relu")
        _bits_same(problems, f"relu forward [{ops.label}]", y, y_ref)
        _bits_same(problems, f"relu backward [{ops.label}]", dd, d_ref)
    _report(problems, f"ReLU n={n}")


@pytest.mark.parametrize("n", FLAT_N)
def test_flat_arena_updates_read_nothing_outside_their_operands(T, n):
    """cnn_sgd_update, cnn_sgd_update_keep, cnn_sgd_momentum_update, cnn_adam_update and cnn_clip_grad_norm: the arena, the gradients, the
    state and `previous` each between poison, bit for bit against the oracle, tests/optim_ref.py and tests/adam_ref.py; read-only
    gradients unchanged"""
    from cnn_amd import capi
    from tests.adam_ref import ref_adam_step, ref_clip, ref_total_norm
    from tests.optim_ref import ref_sgd_step

    lib = capi.load()
    p, g = _flat_data(n, 100 + n), _flat_data(n, 200 + n)
    g[96::97] = 0.0  # (zero gradients; element 0 stays: n = 1 keeps a norm)
    vel, m = _flat_data(n, 300 + n), _flat_data(n, 400 + n)
    v2 = np.abs(_flat_data(n, 500 + n))
    ranges = [(0, 1)] if n < 4 else [(1, n // 2), (n // 2 + 1, n)]  # (they start and end inside 16-byte units, the last one ends at n)
    lr = 1e-2
    sgd_ref = O.sgd_update(p, g, lr)
    sgd8_ref = O.sgd_update(p, g * np.float32(0.125), lr)  # (a power-of-two scale is exact: test_sgd_bit_exact_and_scaled)
    mom = dict(momentum=0.9, weight_decay=1e-2, nesterov=True, grad_scale=0.125)
    pm_ref, vm_ref = ref_sgd_step(p, g, vel, lr, decay_ranges=ranges, **mom)
    adam = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, grad_scale=0.125)
    adam_ref = {dec: ref_adam_step(p, g, m, v2, 3, lr, decoupled=dec, decay_ranges=ranges, **adam) for dec in (False, True)}
    total = ref_total_norm(g)
    n_ws = int(lib.cnn_clip_grad_norm_workspace_bytes(n))
    problems = []
    for poison, shift in FLAT_PLACEMENTS:
        ops = Ops(poison, shift)
        tag = f"[{ops.label}]"
        gd = ops.put("grads", g)
        p1, p2, p3, prev = ops.put("params", p), ops.put("params (scaled)", p), ops.put("params (keep)", p), ops.out("previous", (n,))
        _checked(capi.sgd_update, p1, gd, lr)
        _checked(capi.sgd_update, p2, gd, lr, 0.125)
        _checked(capi.check, lib.cnn_sgd_update_keep(capi._ptr(p3), capi._ptr(gd), n, lr, 1.0, capi._ptr(prev), capi._stream()), "cnn_sgd_update_keep")
        ops.done(T, problems, "sgd_update / sgd_update_keep")
        _bits_same(problems, f"sgd_update {tag}", p1, sgd_ref)
        _bits_same(problems, f"sgd_update, grad_scale 1/8 {tag}", p2, sgd8_ref)
        _bits_same(problems, f"sgd_update_keep params {tag}", p3, sgd_ref)
        _bits_same(problems, f"sgd_update_keep previous {tag}", prev, p)

        ops = Ops(poison, shift)
        gd, pd, vd, prev = ops.put("grads", g), ops.put("params", p), ops.put("velocity", vel), ops.out("previous", (n,))
        _checked(lambda: capi.sgd_momentum_update(pd, gd, vd, lr, decay_ranges=ranges, previous=prev, **mom))
        ops.done(T, problems, "sgd_momentum_update")
        for name, got, want in (("params", pd, pm_ref), ("velocity", vd, vm_ref), ("previous", prev, p), ("grads (read-only)", gd, g)):
            _bits_same(problems, f"sgd_momentum_update {name} {tag}", got, want)

        for dec in (False, True):
            ops = Ops(poison, shift)
            gd, pd, md, vd = ops.put("grads", g), ops.put("params", p), ops.put("exp_avg", m), ops.put("exp_avg_sq", v2)
            prev = ops.out("previous", (n,))
            _checked(lambda: capi.adam_update(pd, gd, md, vd, lr, decoupled=dec, step=3, decay_ranges=ranges, previous=prev, **adam))
            ops.done(T, problems, "adam_update")
            for name, got, want in (("params", pd, adam_ref[dec][0]), ("exp_avg", md, adam_ref[dec][1]), ("exp_avg_sq", vd, adam_ref[dec][2]),
                                    ("previous", prev, p), ("grads (read-only)", gd, g)):
                _bits_same(problems, f"adam_update decoupled={dec} {name} {tag}", got, want)

        # the clip: test_clip_kernel's criterion -- stats[0] the fp64 norm or its fp32 neighbour, the rest ref_clip from the device's stats[0]
        ops = Ops(poison, shift)
        gd, stats = ops.put("grads (in-out)", g), ops.out("stats", (2,))
        ws = guarded.scratch(n_ws, poison=poison, name="clip ws")  # (8-byte aligned by contract: not shifted)
        ops.guards.append(ws)
        _checked(capi.check, lib.cnn_clip_grad_norm(capi._ptr(gd), n, 0.5 * float(total), 1.0, capi._ptr(ws.view), n_ws, capi._ptr(stats), capi._stream()),
                 "cnn_clip_grad_norm")
        ops.done(T, problems, "clip_grad_norm")
        st = host(stats)
        apart = abs(int(st[:1].view(np.uint32)[0]) - int(np.asarray([total], np.float32).view(np.uint32)[0]))
        if not apart <= 1:
            problems.append(f"clip_grad_norm {tag}: total norm {st[0]!r}, fp64 reference {total!r}")
            continue
        want_g, want_coef = ref_clip(g, st[0], 0.5 * float(total))
        _bits_same(problems, f"clip_grad_norm coefficient {tag}", st[1:2], np.asarray([want_coef], np.float32))
        _bits_same(problems, f"clip_grad_norm scaled gradients {tag}", gd, want_g)
    _report(problems, f"flat-arena kernels n={n}")


@pytest.mark.parametrize("n,kind", [(3, "seven"), (1023, "seven")])
def test_layerwise_optimizers_read_nothing_outside_their_operands(T, n, kind):
    """cnn_segment_norms, cnn_lamb_update and cnn_lars_update under tests/test_gpu_layerwise.py's criterion: every norm within one ulp of the
    fp64 value, everything behind the norms bit for bit with tests/lamb_ref.py evaluated from the device's own norms"""
    from cnn_amd import capi
    from tests.lamb_ref import ref_lamb_moments, ref_lamb_step, ref_lars_step, ref_segment_norms
    from tests.test_gpu_layerwise import LAMB, LARS, LR, make_data, make_flags, make_table, ulps

    bounds = make_table(kind, n, 61)
    n_seg = len(bounds) - 1
    assert n_seg >= 3 and n % 2 == 1
    flags = make_flags("mixed", n_seg)
    p, (g,) = make_data(n, bounds, 62, 1)
    m, v = (_flat_data(n, 63) * 0.1).astype(np.float32), (np.abs(_flat_data(n, 64)) * 0.01).astype(np.float32)
    vel = _flat_data(n, 65)
    wd, scale, step = 1e-2, 0.125, 3
    problems = []

    def norms(tag, got, want):
        if not np.all(ulps(got, want) <= 1):
            problems.append(f"{tag}: a norm is {int(ulps(got, want).max())} ulps from the fp64 value")

    for poison, shift in FLAT_PLACEMENTS:
        lw = capi.Layerwise(bounds, flags)
        ops = Ops(poison, shift)
        tag = f"[{ops.label}]"
        xd, out = ops.put("x", p), ops.out("norms", (n_seg,))
        _checked(lw.segment_norms, xd, out)
        ops.done(T, problems, "segment_norms")
        norms(f"segment_norms {tag}", host(out), ref_segment_norms(p, bounds))

        ops = Ops(poison, shift)
        pd, gd, md, vd = ops.put("params", p), ops.put("grads", g), ops.put("exp_avg", m), ops.put("exp_avg_sq", v)
        ud, prev = ops.out("update", (n,)), ops.out("previous", (n,))
        _checked(lambda: lw.lamb_update(pd, gd, md, vd, ud, LR, weight_decay=wd, step=step, grad_scale=scale, previous=prev, **LAMB))
        ops.done(T, problems, "lamb_update")
        wn, un, ratio = lw.stats()
        r, _, _ = ref_lamb_moments(p, g, m, v, bounds, flags, step, weight_decay=wd, grad_scale=scale, **LAMB)
        norms(f"lamb w_norm {tag}", wn, ref_segment_norms(p, bounds))
        norms(f"lamb u_norm {tag}", un, ref_segment_norms(r, bounds))
        if np.all(np.isfinite(wn)) and np.all(np.isfinite(un)):
            want = ref_lamb_step(p, g, m, v, bounds, flags, step, LR, wn, un, weight_decay=wd, grad_scale=scale, **LAMB)
            for name, got, ref_ in (("params", pd, want[0]), ("exp_avg", md, want[1]), ("exp_avg_sq", vd, want[2]), ("update", ud, want[3]),
                                    ("ratio", ratio, want[4]), ("previous", prev, p), ("grads (read-only)", gd, g)):
                _bits_same(problems, f"lamb_update {name} {tag}", got, np.asarray(ref_, np.float32))

        ops = Ops(poison, shift)
        pd, gd, vd, prev = ops.put("params", p), ops.put("grads", g), ops.put("velocity", vel), ops.out("previous", (n,))
        _checked(lambda: lw.lars_update(pd, gd, vd, LR, weight_decay=wd, nesterov=True, grad_scale=scale, previous=prev, **LARS))
        ops.done(T, problems, "lars_update")
        wn, un, ratio = lw.stats()
        norms(f"lars w_norm {tag}", wn, ref_segment_norms(p, bounds))
        norms(f"lars u_norm {tag}", un, ref_segment_norms(g, bounds) * np.float32(scale))  # (1/8: exact, still one ulp)
        if np.all(np.isfinite(wn)) and np.all(np.isfinite(un)):
            want_p, want_v, want_gnt, want_ratio = ref_lars_step(p, g, vel, bounds, flags, LR, wn, un, weight_decay=wd, nesterov=True, grad_scale=scale,
                                                                 norm_is_scaled=True, **LARS)
            for name, got, ref_ in (("params", pd, want_p), ("velocity", vd, want_v), ("u_norm", un, want_gnt), ("ratio", ratio, want_ratio),
                                    ("previous", prev, p), ("grads (read-only)", gd, g)):
                _bits_same(problems, f"lars_update {name} {tag}", got, np.asarray(ref_, np.float32))
        lw.close()
    _report(problems, f"layer-wise optimizers n={n}, {n_seg} segments")


@pytest.mark.parametrize("B,n_in,n_out", [(1, 1, 1), (3, 37, 3), (5, 256, 3), (2, 515, 8), (7, 1029, 10)])
def test_linear_layer_reads_nothing_outside_its_operands(T, B, n_in, n_out):
    """cnn_linear_forward / _backward at test_linear_vs_oracle's criterion (REL_TOL against the oracle); cnn_linear_backward_relu and the two
    fused heads (out <= 8) at their bit-identity tests' criterion: the unfused sequence under the same placement, bit for bit"""
    from cnn_amd import capi
    from tests.test_gpu_scratch_contract import _close

    lib, P, S = capi.load(), capi._ptr, capi._stream
    x = np.maximum(uniform_pm1(10, (B, n_in)), np.float32(0))  # (a ReLU layer's output: zeros where backward_relu masks)
    w, b, dy = normal_scaled(11, (n_in, n_out)), normal_scaled(12, (n_out,)), uniform_pm1(13, (B, n_out))
    labels = (np.arange(B) % n_out).astype(np.int32)
    y_ref = O.linear_forward(x, w, b)
    gw_ref, gb_ref, dx_ref = O.linear_backward(x, dy, w)
    problems = []
    for poison, shift in THREE:
        ops = Ops(poison, shift)
        tag = f"[{ops.label}]"
        xd, wd, bd, dyd, ld = ops.put("x", x), ops.put("w", w), ops.put("bias", b), ops.put("dy", dy), ops.put("labels", labels)
        y = ops.out("y", (B, n_out))
        gw, gb, dx = ops.out("gw", (n_in, n_out)), ops.out("gb", (n_out,)), ops.out("dx", (B, n_in))
        gw2, gb2, dx2 = ops.out("gw (relu)", (n_in, n_out)), ops.out("gb (relu)", (n_out,)), ops.out("dx (relu)", (B, n_in))
        _checked(capi.linear_forward, xd, wd, bd, y)
        _checked(capi.linear_backward, xd, dyd, wd, float(B), gw, gb, dx)
        _checked(capi.linear_backward, xd, dyd, wd, float(B), gw2, gb2, dx2, True)
        ops.done(T, problems, "linear forward / backward / backward_relu")
        for name, got, want in (("forward", y, y_ref), ("gW", gw, gw_ref), ("gb", gb, gb_ref), ("dx", dx, dx_ref)):
            _close(problems, f"linear {name} {tag}", host(got), want)
        _bits_same(problems, f"backward_relu gW == backward's {tag}", gw2, host(gw))
        _bits_same(problems, f"backward_relu gb == backward's {tag}", gb2, host(gb))
        _bits_same(problems, f"backward_relu dx == backward + relu_backward {tag}", dx2, O.relu_backward(x, host(dx)))
        if n_out > 8:  # (the fused heads: out <= 8)
            continue
        # the heads: cnn_linear_forward + cnn_softmax_xent, then the fused forms, every tensor of every call between poison
        mk = lambda name, *shape: ops.out(name, shape)
        probs0, delta0, loss0 = mk("probs", B, n_out), mk("delta", B, n_out), mk("loss", 1)
        _checked(capi.check, lib.cnn_softmax_xent(P(y), P(ld), P(probs0), P(delta0), P(loss0), B, n_out, S()), "cnn_softmax_xent")
        gw0, gb0, dx0 = mk("gw of delta", n_in, n_out), mk("gb of delta", n_out), mk("dx of delta", B, n_in)
        _checked(capi.linear_backward, xd, delta0, wd, float(B), gw0, gb0, dx0, True)
        logits1, probs1, delta1, terms1, loss1 = mk("head logits", B, n_out), mk("head probs", B, n_out), mk("head delta", B, n_out), mk("head terms", B), mk("head loss", 1)
        _checked(capi.check, lib.cnn_linear_forward_softmax_xent(P(xd), P(wd), P(bd), P(ld), P(logits1), P(probs1), P(delta1), P(terms1), B, n_in, n_out, S()),
                 "cnn_linear_forward_softmax_xent")
        _checked(capi.check, lib.cnn_loss_from_terms(P(terms1), P(loss1), B, S()), "cnn_loss_from_terms")
        logits2, probs2, delta2, terms2, dxh = mk("dx-head logits", B, n_out), mk("dx-head probs", B, n_out), mk("dx-head delta", B, n_out), mk("dx-head terms", B), mk("dx-head dx", B, n_in)
        _checked(capi.check, lib.cnn_linear_forward_softmax_xent_dx(P(xd), P(wd), P(bd), P(ld), P(logits2), P(probs2), P(delta2), P(terms2), P(dxh), 1, B, n_in,
                                                                   n_out, S()), "cnn_linear_forward_softmax_xent_dx")
        gwh, gbh = mk("gw (dx == NULL)", n_in, n_out), mk("gb (dx == NULL)", n_out)
        _checked(capi.check, lib.cnn_linear_backward(P(xd), P(delta2), P(wd), P(gwh), P(gbh), None, B, n_in, n_out, float(B), S()), "cnn_linear_backward")
        ops.done(T, problems, "the fused heads")
        for name, a, c in (("logits", y, logits1), ("probs", probs0, probs1), ("delta", delta0, delta1), ("loss", loss0, loss1),
                           ("logits (dx head)", y, logits2), ("probs (dx head)", probs0, probs2), ("delta (dx head)", delta0, delta2),
                           ("loss terms (dx head)", terms1, terms2), ("dx (dx head)", dx0, dxh), ("gW (dx == NULL)", gw0, gwh), ("gb (dx == NULL)", gb0, gbh)):
            _bits_same(problems, f"head {name} {tag}", c, host(a))
        # ... and the unfused head itself against the oracle (test_softmax_xent_vs_oracle's bounds on the oracle's softmax of the device's logits)
        p_ref = O.softmax(host(y))
        _, d_ref = O.cross_entropy_backward(p_ref, labels)
        if not (np.allclose(host(probs0), p_ref, rtol=1e-5, atol=1e-7) and np.allclose(host(delta0), d_ref, rtol=1e-5, atol=1e-6)):
            problems.append(f"head probs / delta {tag}: not the oracle's softmax of these logits")
    _report(problems, f"LinearLayer B {B}, {n_in} -> {n_out}")


@pytest.mark.parametrize("classes", [1, 3, 10])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_softmax_xent_reads_nothing_outside_its_operands(T, B, classes):
    """test_softmax_xent_vs_oracle's criteria; `labels` is an int32 operand between poison (0x5A5A5A5A as a label: a huge index)"""
    from cnn_amd import capi

    lib, P, S = capi.load(), capi._ptr, capi._stream
    logits = (uniform_pm1(16, (B, classes)) * 12).astype(np.float32)
    logits[0] = 0
    labels = ((np.arange(B) * 7 + 2) % classes).astype(np.int32)
    p_ref = O.softmax(logits)
    loss_ref, d_ref = O.cross_entropy_backward(p_ref, labels)
    assert np.isfinite(loss_ref)
    problems = []
    for poison, shift in THREE:
        ops = Ops(poison, shift)
        ld, lab = ops.put("logits", logits), ops.put("labels", labels)
        probs, delta, loss = ops.out("probs", (B, classes)), ops.out("delta", (B, classes)), ops.out("loss", (1,))
        delta2 = ops.out("delta (probs, loss == NULL)", (B, classes))
        _checked(capi.check, lib.cnn_softmax_xent(P(ld), P(lab), P(probs), P(delta), P(loss), B, classes, S()), "cnn_softmax_xent")
        _checked(capi.check, lib.cnn_softmax_xent(P(ld), P(lab), None, P(delta2), None, B, classes, S()), "cnn_softmax_xent")
        ops.done(T, problems, "softmax_xent")
        if not np.allclose(host(probs), p_ref, rtol=1e-5, atol=1e-7):
            problems.append(f"probs [{ops.label}]: beyond rtol 1e-5, atol 1e-7 of the oracle")
        if not np.allclose(host(delta), d_ref, rtol=1e-5, atol=1e-6):
            problems.append(f"delta [{ops.label}]: beyond rtol 1e-5, atol 1e-6 of the oracle")
        if not np.isclose(float(host(loss)[0]) / B, loss_ref, rtol=1e-5):
            problems.append(f"loss [{ops.label}]: {float(host(loss)[0]) / B!r}, the oracle's {loss_ref!r}")
        _bits_same(problems, f"delta without probs and loss [{ops.label}]", delta2, host(delta))
    _report(problems, f"softmax_xent B {B}, {classes} classes")


@pytest.mark.parametrize("shape,p", [((2, 5, 3, 7), 0.29), ((1, 17, 6, 6), 0.5)])
def test_dropout_and_grad_cam_read_nothing_outside_their_operands(T, shape, p):
    """bit for bit against the oracle, as tests/sweeps/fuzz_layers.py (misc) compares them"""
    from cnn_amd import capi

    x = uniform_pm1(21, shape)
    f = np.abs(x)
    want = {"train": O.dropout_forward(x, p, training=True), "eval": O.dropout_forward(x, p, training=False), "backward": O.dropout_backward(x, p)}
    cam_ref, img_ref = O.grad_cam(f)
    B, Cc, H, W = shape
    problems = []
    for poison, shift in THREE:
        ops = Ops(poison, shift)
        xd, y1, y2, dd = ops.put("x", x), ops.out("y (training)", shape), ops.out("y (eval)", shape), ops.put("dy (in-out)", x)
        _checked(capi.dropout_forward, xd, p, True, y1)
        _checked(capi.dropout_forward, xd, p, False, y2)
        _checked(capi.dropout_backward, dd, p)
        fd, cam, img = ops.put("feature", f), ops.out("cam", (B, H, W)), ops.out("picture", (H, W), T.uint8)
        _checked(capi.check, capi.load().cnn_grad_cam(capi._ptr(fd), B, Cc, H, W, capi._ptr(cam), capi._ptr(img), capi._stream()), "cnn_grad_cam")
        ops.done(T, problems, "dropout / grad_cam")
        for name, got, ref_ in (("dropout forward (training)", y1, want["train"]), ("dropout forward (eval)", y2, want["eval"]),
                                ("dropout backward", dd, want["backward"]), ("grad-cam map", cam, cam_ref), ("grad-cam picture", img, img_ref)):
            _bits_same(problems, f"{name} [{ops.label}]", got, ref_)
    _report(problems, f"Dropout / Grad-CAM {shape}")


# ---- BatchNorm2D: the sibling module's calls and criteria, the operands guarded (shift 0 only: the header asks for 16- / 8-byte alignment) ----
from tests.test_gpu_batchnorm import BN_SHAPES, POOLED_SHAPES  # noqa: E402
from tests.test_gpu_scratch_contract import _batchnorm_calls  # noqa: E402


@pytest.mark.parametrize("shape", BN_SHAPES[:4] + POOLED_SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_reads_nothing_outside_its_operands(T, shape):
    """training forward (+ ReLU), eval forward, backward, the fused pool forward, the pooled-domain backward and the four sync-BN phases:
    x, gamma, beta, the moving and saved statistics, dpool, mask and pooled between NaNs and between 0x5A bytes"""
    _batchnorm_calls(T, shape, guard_operands=True)
