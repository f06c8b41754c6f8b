"""LAMB and LARS without a GPU: the NumPy restatements of both updates (tests/lamb_ref.py) against independent fp64 restatements and
against the momentum-SGD reference, the special cases of the trust ratio, the new entry points' exports and bindings, and the argument
checks that come before any allocation or launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.lamb_ref import (SEG_ADAPT, SEG_DECAY, lamb_host_scalars, ref_lamb_moments, ref_lamb_ratio, ref_lamb_step, ref_lars_ratio,
                            ref_lars_step, ref_segment_norms, segment_table_of)
from tests.optim_ref import decay_ranges_of, ref_sgd_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24  # the unit roundoff of fp32: one rounding moves a value by at most U times its magnitude


def arena(n, seed, n_seg=9):
    """parameters, gradients (every 97th exactly 0), a table of n_seg segments with mixed flags; segment 1 has zero gradients, segment 2
    zero parameters"""
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    grads = [rs.standard_normal(n).astype(np.float32) for _ in range(3)]
    cuts = np.sort(rs.choice(np.arange(1, n), n_seg - 1, replace=False))
    bounds = np.concatenate([[0], cuts, [n]]).astype(np.uint32)
    flags = np.array([(SEG_DECAY | SEG_ADAPT, SEG_ADAPT, SEG_DECAY, 0)[s % 4] for s in range(n_seg)], np.uint32)
    flags[1] = flags[2] = SEG_DECAY | SEG_ADAPT
    for g in grads:
        g[::97] = 0.0
        g[bounds[1]:bounds[2]] = 0.0
    p[bounds[2]:bounds[3]] = 0.0
    return p, grads, bounds, flags


def spread(values, bounds):
    return np.repeat(np.asarray(values), np.diff(np.asarray(bounds, np.int64)))


def test_lars_reference_without_adapt_is_momentum_sgd_bit_for_bit():
    n = 4099
    p, grads, bounds, flags = arena(n, 11)
    flags = flags & SEG_DECAY
    ranges = [(int(bounds[s]), int(bounds[s + 1])) for s in range(len(flags)) if flags[s] & SEG_DECAY]
    for momentum, wd, nesterov, scale in [(0.0, 0.0, False, 1.0), (0.9, 0.0, False, 1.0), (0.9, 5e-4, False, 0.125), (0.9, 5e-4, True, 1.0),
                                          (0.0, 1e-2, False, 0.125)]:
        pa, va = p.copy(), np.zeros(n, np.float32)
        pb, vb = p.copy(), np.zeros(n, np.float32)
        for g in grads:
            wn, gn = ref_segment_norms(pa, bounds), ref_segment_norms(g, bounds)
            pa, va, _, ratio = ref_lars_step(pa, g, va, bounds, flags, 0.05, wn, gn, momentum, wd, 1e-3, 1e-8, nesterov, scale)
            pb, vb = ref_sgd_step(pb, g, vb, 0.05, momentum, wd, nesterov, scale, ranges)
            assert np.all(ratio == np.float32(1))
            assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
        assert np.abs(pa - p).max() > 1e-3


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_lamb_reference_against_fp64(wd, scale):
    """Three steps (the state carries) against the same formulas in float64, fed the SAME fp32 inputs, host scalars and ratios at every
    step, so the difference is the fp32 rounding of one step's chain.  With U = 2^-24 and A the value of r with every term taken
    by magnitude (no cancellation: A = (beta1|m| + omb1|gs|) / bc1 / den + wd|p|):
      den  : v' is a sum of non-negative terms, 4 roundings (<= 4U), the root halves that and adds 1, / bc2s and + eps add 1 each: <= 5U
      r    : gs, beta1*m, omb1*gs, their sum, / bc1, / den: 6U of the magnitudes, + den's 5U, + wd*p and the last sum: <= 13U * A
      p'   : ratio*r and lr*t round once each (2U), the subtraction rounds to U * |p'| <= U * (|p| + lr*ratio*A)
    => |r - r64| <= 16U * A and |p' - p'64| <= U * |p| + 20U * lr * ratio * A, with room for the second-order terms: a few ulps of
    the step.  m' and v' are held to 4U of their magnitude sums."""
    n, lr, b1, b2, eps = 4099, 0.02, 0.9, 0.999, 1e-6
    p, grads, bounds, flags = arena(n, 5)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for step, g in enumerate(grads, start=1):
        wn = ref_segment_norms(p, bounds)
        r, _, _ = ref_lamb_moments(p, g, m, v, bounds, flags, step, b1, b2, eps, wd, scale)
        un = ref_segment_norms(r, bounds)
        p_new, m_new, v_new, r2, ratio = ref_lamb_step(p, g, m, v, bounds, flags, step, lr, wn, un, b1, b2, eps, wd, scale)
        assert np.array_equal(r, r2)
        # float64, from the same fp32 values
        omb1, omb2, bc2s, bc1 = (float(x) for x in lamb_host_scalars(step, b1, b2))
        fb1, fb2, feps, fwd, fs, flr = (float(np.float32(x)) for x in (b1, b2, eps, wd, scale, lr))
        P, G, M, V = (a.astype(np.float64) for a in (p, g, m, v))
        GS = G * fs
        M64 = fb1 * M + omb1 * GS
        V64 = fb2 * V + omb2 * GS * GS
        DEN = np.sqrt(V64) / bc2s + feps
        dec = spread((flags & SEG_DECAY) != 0, bounds) & (wd != 0)
        R64 = M64 / bc1 / DEN + np.where(dec, fwd * P, 0.0)
        A = (fb1 * np.abs(M) + omb1 * np.abs(GS)) / bc1 / DEN + np.where(dec, fwd * np.abs(P), 0.0)
        RAT = spread(ratio, bounds).astype(np.float64)
        P64 = P - flr * RAT * R64
        assert np.all(np.abs(m_new - M64) <= 4 * U * (fb1 * np.abs(M) + omb1 * np.abs(GS)))
        assert np.all(np.abs(v_new - V64) <= 4 * U * V64)
        assert np.all(np.abs(r - R64) <= 16 * U * A)
        bound = U * np.abs(P) + 20 * U * flr * RAT * A
        err = np.abs(p_new - P64)
        assert np.all(err <= bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        # the ratio: one rounding of w / u where it applies
        use = ((flags & SEG_ADAPT) != 0) & (wn > 0) & (un > 0)
        assert np.all(ratio[~use] == np.float32(1))
        assert np.all(np.abs(ratio[use] - wn[use].astype(np.float64) / un[use].astype(np.float64)) <= U * ratio[use])
        p, m, v = p_new, m_new, v_new
    print(f"LAMB wd={wd} scale={scale}: worst error {worst:.3f} of the bound")
    assert worst > 0.0


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("wd,scale", [(0.0, 1.0), (5e-4, 0.125)])
def test_lars_reference_against_fp64(wd, scale, nesterov):
    """As above for LARS.  With D = |gs| + wd|p| and r the segment's ratio:
      d   : gs, wd*p, the sum: <= 3U * D;  dl = r * d: <= 4U * r*D
      v'  : momentum*v rounds once, the sum once: <= 5U * r*D + 2U * mom*|v|
      u   : v' itself, or dl + momentum*v' (two more roundings): <= 7U * Uabs with Uabs = r*D + mom*|v| (plain) or
            r*D*(1 + mom) + mom^2*|v| (Nesterov)
      p'  : lr*u rounds once, the subtraction to U * |p'|
    => |p' - p'64| <= U * |p| + 12U * lr * Uabs and |v' - v'64| <= 6U * (r*D + mom*|v|).  The ratio is five roundings of positive
    terms: 8U relative."""
    n, lr, mom, tc, eps = 4099, 0.5, 0.9, 1e-3, 1e-8
    p, grads, bounds, flags = arena(n, 6)
    v = np.zeros(n, np.float32)
    worst = 0.0
    for g in grads:
        wn, gn = ref_segment_norms(p, bounds), ref_segment_norms(g, bounds)
        p_new, v_new, gnt, ratio = ref_lars_step(p, g, v, bounds, flags, lr, wn, gn, mom, wd, tc, eps, nesterov, scale)
        flr, fmom, fwd, fs, ftc, feps = (float(np.float32(x)) for x in (lr, mom, wd, scale, tc, eps))
        P, G, V = (a.astype(np.float64) for a in (p, g, v))
        GS = G * fs
        dec = spread((flags & SEG_DECAY) != 0, bounds) & (wd != 0)
        Dv = GS + np.where(dec, fwd * P, 0.0)
        Dabs = np.abs(GS) + np.where(dec, fwd * np.abs(P), 0.0)
        RAT = spread(ratio, bounds).astype(np.float64)
        V64 = fmom * V + RAT * Dv
        U64 = RAT * Dv + fmom * V64 if nesterov else V64
        P64 = P - flr * U64
        Vabs = RAT * Dabs + fmom * np.abs(V)
        Uabs = RAT * Dabs + fmom * Vabs if nesterov else Vabs
        assert np.all(np.abs(v_new - V64) <= 6 * U * Vabs)
        bound = U * np.abs(P) + 12 * U * flr * Uabs
        err = np.abs(p_new - P64)
        assert np.all(err <= bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        W, GN = wn.astype(np.float64), gn.astype(np.float64) * fs
        wds = np.where((flags & SEG_DECAY) != 0, fwd, 0.0)
        use = ((flags & SEG_ADAPT) != 0) & (wn > 0) & (gnt > 0)
        want = ftc * W / (GN + wds * W + feps)
        assert np.all(ratio[~use] == np.float32(1))
        assert np.all(np.abs(ratio[use] - want[use]) <= 8 * U * want[use])
        assert np.all(np.abs(gnt - GN) <= U * GN)
        p, v = p_new, v_new
    print(f"LARS wd={wd} scale={scale} nesterov={nesterov}: worst error {worst:.3f} of the bound")
    assert worst > 0.0


def test_zero_norm_segments_have_ratio_one():
    n = 2000
    p, grads, bounds, flags = arena(n, 8)
    g = grads[0]
    z = np.zeros(n, np.float32)
    zero_g, zero_p = slice(int(bounds[1]), int(bounds[2])), slice(int(bounds[2]), int(bounds[3]))
    wn = ref_segment_norms(p, bounds)
    assert wn[2] == 0 and np.all(np.delete(wn, 2) > 0)
    # LAMB, no decay: zero gradient on a zero state gives r = 0, u_norm = 0, ratio 1, parameters untouched
    r, _, _ = ref_lamb_moments(p, g, z, z, bounds, flags, 1)
    un = ref_segment_norms(r, bounds)
    p1, m1, v1, _, ratio = ref_lamb_step(p, g, z, z, bounds, flags, 1, 0.1, wn, un)
    assert un[1] == 0 and ratio[1] == np.float32(1) and ratio[2] == np.float32(1)
    assert np.array_equal(p1[zero_g].view(np.uint32), p[zero_g].view(np.uint32)) and not np.any(m1[zero_g]) and not np.any(v1[zero_g])
    # zero parameters: the step is Adam's bias-corrected one, ratio 1
    assert np.array_equal(p1[zero_p], (np.float32(0) - np.float32(0.1) * (np.float32(1) * r))[zero_p]) and np.any(p1[zero_p])
    adapted = [s for s in range(len(flags)) if flags[s] & SEG_ADAPT and s not in (1, 2)]
    assert adapted and all(ratio[s] == np.float32(wn[s] / un[s]) for s in adapted)
    assert all(ratio[s] == np.float32(1) for s in range(len(flags)) if not flags[s] & SEG_ADAPT)
    assert np.array_equal(ref_lamb_ratio(wn, un, np.zeros_like(flags)), np.ones(len(flags), np.float32))
    # LARS
    gn = ref_segment_norms(g, bounds)
    p2, _, gnt, ratio = ref_lars_step(p, g, z, bounds, flags, 0.1, wn, gn, 0.9, 5e-4)
    assert gn[1] == 0 and ratio[1] == np.float32(1) and ratio[2] == np.float32(1)
    assert all(0 < ratio[s] < 1 for s in adapted)
    assert np.array_equal(gnt, gn) and np.array_equal(ref_lars_ratio(wn, gn, flags, 5e-4, grad_scale=0.125)[0], gn * np.float32(0.125))


def test_moving_statistics_segments_come_back_unchanged():
    """BatchNorm2D's moving statistics share the arena: zero gradient, zero state, no flags -- neither optimizer moves them, whatever
    the weight decay"""
    from cnn_amd import stacks

    layout = stacks.walk(stacks.alexnet(3, batch_norm=True), 3, 224, 224)
    for decay_small, adapt_small in [(False, False), (True, True)]:
        bounds, flags = segment_table_of(layout, decay_small, adapt_small)
        n = int(bounds[-1])
        assert n == sum(e["params"] for e in layout)
        moving = np.zeros(n, bool)
        off = 0
        for e in layout:
            if e["kind"] == "bn":
                moving[off + e["params"] // 2:off + e["params"]] = True
            off += e["params"]
        assert moving.any() and not np.any(spread(flags, bounds)[moving])
        # the DECAY flags are the existing decay policy
        ranges = decay_ranges_of(layout, decay_small)
        inside = np.zeros(n, bool)
        for b, e in ranges:
            inside[b:e] = True
        assert np.array_equal(spread((flags & SEG_DECAY) != 0, bounds), inside)
        rs = np.random.RandomState(2)
        p = rs.standard_normal(n).astype(np.float32)
        g = rs.standard_normal(n).astype(np.float32)
        g[moving] = 0.0
        z = np.zeros(n, np.float32)
        wn = ref_segment_norms(p, bounds)
        r, _, _ = ref_lamb_moments(p, g, z, z, bounds, flags, 1, weight_decay=1e-2)
        p1, m1, v1, _, _ = ref_lamb_step(p, g, z, z, bounds, flags, 1, 0.1, wn, ref_segment_norms(r, bounds), weight_decay=1e-2)
        assert np.array_equal(p1[moving].view(np.uint32), p[moving].view(np.uint32)) and not np.any(m1[moving]) and not np.any(v1[moving])
        assert np.all(p1[~moving] != p[~moving])
        p2, v2, _, _ = ref_lars_step(p, g, z, bounds, flags, 0.1, wn, ref_segment_norms(g, bounds), 0.9, 5e-4)
        assert np.array_equal(p2[moving].view(np.uint32), p[moving].view(np.uint32)) and not np.any(v2[moving])


def test_new_symbols_are_exported_declared_and_bound():
    from cnn_amd import capi, hostapi

    names = ["cnn_layerwise_create", "cnn_layerwise_destroy", "cnn_layerwise_stats", "cnn_segment_norms", "cnn_lamb_update", "cnn_lars_update"]
    hdr = open(os.path.join(ROOT, "include", "cnn_amd.h")).read()
    lib = capi.load()
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.cnn_amd_abi_version() == 2
    assert C.sizeof(capi.LambOptions) == 32 and C.sizeof(capi.LarsOptions) == 24
    host = hostapi.load()
    for name in ["cnnh_net_set_lamb", "cnnh_net_set_lars", "cnnh_net_segment_count", "cnnh_net_get_segments", "cnnh_net_get_trust_stats"]:
        assert hasattr(host, name), name


def test_bad_tables_and_arguments_are_refused_before_anything_is_allocated():
    from cnn_amd import capi

    lib = capi.load()

    def create(bounds, flags):
        b, f = np.asarray(bounds, np.uint32), np.asarray(flags, np.uint32)
        h = C.c_void_p()
        rc = lib.cnn_layerwise_create(b.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), len(flags), C.byref(h))
        return rc, h.value, lib.cnn_amd_last_error().decode()

    for bounds, flags in [([0, 10, 10, 20], [0, 0, 0]),        # an empty segment
                          ([0, 10, 5, 20], [0, 0, 0]),         # unsorted
                          ([1, 10], [0]),                      # does not start at 0
                          ([0, 10], [4]),                      # an unknown flag
                          ([0, 2 ** 32 - 256], [0]),           # beyond the 32-bit limit
                          ([0], [])]:                          # no segment
        rc, h, msg = create(bounds, flags)
        assert rc != 0 and h is None and "cnn_layerwise_create" in msg, (bounds, rc, msg)
    with pytest.raises(capi.CnnAmdError):
        capi.Layerwise([0, 4, 8], [0])  # (the table's two arrays disagree)
    # no handle: every entry point answers with a status and a message
    opt = capi.LambOptions(1e-3, 0.9, 0.999, 1e-6, 0.0, 1)
    assert lib.cnn_lamb_update(None, None, None, None, None, None, C.byref(opt), 1.0, None, None) != 0
    assert "cnn_lamb_update" in lib.cnn_amd_last_error().decode()
    lopt = capi.LarsOptions(1e-3, 0.9, 0.0, 1e-3, 1e-8, 0)
    assert lib.cnn_lars_update(None, None, None, None, C.byref(lopt), 1.0, None, None) != 0
    assert "cnn_lars_update" in lib.cnn_amd_last_error().decode()
    assert lib.cnn_segment_norms(None, None, None, None) != 0 and lib.cnn_layerwise_destroy(None) != 0
    assert lib.cnn_layerwise_stats(None, None) != 0
