"""The parameter average without a device: cnn_ema_decay_at against the NumPy restatement (tests/ema_ref.py), properties of the
restatement itself, the new symbols of both libraries, and the refusals of cnn_ema_update / cnn_arena_swap, which come before any
launch (host memory is enough)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.ema_ref import merged, ref_ema_decay_at, ref_ema_update
from tests.test_gpu_grad_accumulate import PAIRS

DECAYS = (0.9, 0.999, 0.9999)
TS = (0, 1, 2, 9, 10, 89, 90, 9989, 9990, 10**6, 2**40)


def word(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("decay", DECAYS)
def test_decay_at_equals_the_restatement(decay):
    from cnn_amd import capi

    lib = capi.load()
    for warmup in (0, 1):
        got = [lib.cnn_ema_decay_at(decay, warmup, t) for t in TS]
        want = [ref_ema_decay_at(decay, warmup, t) for t in TS]
        assert [word(g) for g in got] == [word(w) for w in want], (decay, warmup, got, want)
        assert [capi.ema_decay_at(decay, warmup, t) for t in TS] == got
        if not warmup:
            assert all(word(g) == word(decay) for g in got)
    seq = [lib.cnn_ema_decay_at(decay, 1, t) for t in range(0, 100001)]
    assert word(seq[0]) == word(0.1)
    assert all(a <= b for a, b in zip(seq, seq[1:])), "the warm-up never decreases"
    assert word(seq[-1]) == word(decay) and word(lib.cnn_ema_decay_at(decay, 1, 2**40)) == word(decay)
    assert all(s <= np.float32(decay) for s in seq)


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_restatement_keeps_a_constant_vector():
    """shadow == parameters == c: decay * c + (1 - decay) * c is c up to the three roundings.  Measured here: an update moves an
    element by at most 1 ulp -- the first update does move some by exactly 1 ulp for these decays, the later ones by none -- so after
    k updates the shadow is within 1 ulp of c, well inside k ulp"""
    rs = np.random.RandomState(0)
    c = (rs.standard_normal(200000) * np.exp(rs.uniform(-20, 20, 200000))).astype(np.float32)
    for decay in DECAYS + (0.5,):
        e = c.copy()
        for k in range(1, 6):
            nxt = ref_ema_update(e, c, decay, [(0, c.size)])
            step, drift = int(ulps(nxt, e).max()), int(ulps(nxt, c).max())
            print(f"decay {decay} update {k}: moved by {step} ulp, {drift} ulp from the constant")
            assert step <= 1 and drift <= 1
            if k == 1:
                assert step == (0 if decay == 0.5 else 1)
            else:
                assert step == 0
            e = nxt


def test_restatement_copies_bits():
    """decay 0, and every element outside the ranges: the output words are the parameters' words, whatever the shadow held"""
    a = np.array([p[0] for p in PAIRS], np.uint32).view(np.float32)
    b = np.array([p[1] for p in PAIRS], np.uint32).view(np.float32)
    out = ref_ema_update(a, b, 0.0, [(0, a.size)])
    assert np.array_equal(out.view(np.uint32), b.view(np.uint32))
    out = ref_ema_update(None, b, 0.0, [])
    assert np.array_equal(out.view(np.uint32), b.view(np.uint32))
    out = ref_ema_update(a, b, 0.9, [(3, 5)])
    keep = np.ones(a.size, bool)
    keep[3:5] = False
    assert np.array_equal(out.view(np.uint32)[keep], b.view(np.uint32)[keep])
    assert merged([(0, 4), (4, 9), (12, 13), (13, 20)]) == [(0, 9), (12, 20)]


def test_new_symbols_are_exported_declared_and_bound():
    from cnn_amd import capi, hostapi

    P = C.c_void_p
    assert capi.SIGNATURES["cnn_ema_decay_at"] == (C.c_float, [C.c_float, C.c_int, C.c_uint64])
    assert capi.SIGNATURES["cnn_ema_update"] == (C.c_int, [P, P, C.c_size_t, C.c_float, P, P, C.c_size_t, P])
    assert capi.SIGNATURES["cnn_arena_swap"] == (C.c_int, [P, P, C.c_size_t, P])
    lib = capi.load()
    for name in ("cnn_ema_decay_at", "cnn_ema_update", "cnn_arena_swap"):
        assert hasattr(lib, name)
    assert lib.cnn_amd_abi_version() == 2
    syms = subprocess.run(["nm", "-D", "--defined-only", hostapi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("cnnh_net_set_ema", "cnnh_net_reset_ema", "cnnh_net_get_ema", "cnnh_net_ema_updates", "cnnh_net_swap_ema", "cnnh_net_ema_swapped",
                 "cnnh_net_save_ema_state", "cnnh_net_load_ema_state"):
        assert f" T {name}\n" in syms, name
        assert name in hostapi.SIGNATURES, name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cnn_amd.h")).read()
    assert "cnn_ema_update(float* ema, const float* params, size_t n, float decay, const uint32_t* avg_ranges" in hdr


def fptr(a):
    return C.c_void_p(a.ctypes.data)


def table(ranges):
    t = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1, 2))
    return t, C.c_void_p(t.ctypes.data)


def test_ema_update_refuses_before_any_launch():
    from cnn_amd import capi

    lib = capi.load()
    n = 1000
    buf = np.zeros(2 * n + 8, np.float32)
    ema, p = buf[:n], buf[n:2 * n]
    before = buf.copy()
    one, one_p = table([(0, n)])
    unsorted, unsorted_p = table([(10, 20), (5, 8)])
    beyond, beyond_p = table([(0, 10), (990, n + 1)])
    many, many_p = table([(2 * k, 2 * k + 1) for k in range(65)])
    nan = float("nan")
    cases = [
        ((None, fptr(p), n, 0.5, one_p, None, 1), b"null"),
        ((fptr(ema), None, n, 0.5, one_p, None, 1), b"null"),
        ((fptr(ema), fptr(p), 0, 0.5, None, None, 0), b"n=0"),
        ((fptr(ema), fptr(ema), n, 0.5, one_p, None, 1), b"overlap"),
        ((fptr(ema), fptr(buf[n - 1:]), n, 0.5, one_p, None, 1), b"overlap"),
        ((fptr(buf[1:]), fptr(ema), n, 0.0, None, None, 0), b"overlap"),
        ((fptr(ema), fptr(p), n, 1.0, one_p, None, 1), b"decay"),
        ((fptr(ema), fptr(p), n, -0.1, one_p, None, 1), b"decay"),
        ((fptr(ema), fptr(p), n, nan, one_p, None, 1), b"decay"),
        ((fptr(ema), fptr(p), n, 0.5, unsorted_p, None, 2), b"range 1"),
        ((fptr(ema), fptr(p), n, 0.5, beyond_p, None, 2), b"range 1"),
        ((fptr(ema), fptr(p), n, 0.5, many_p, None, 65), b"CNN_SGD_INLINE_RANGES"),
        ((fptr(ema), fptr(p), n, 0.5, None, None, 1), b"null"),
    ]
    for args, needle in cases:
        assert lib.cnn_ema_update(*args, None) == 1, args
        msg = lib.cnn_amd_last_error()
        assert msg.startswith(b"cnn_ema_update") and needle in msg, (args, msg)
    assert np.array_equal(buf, before)
    assert (unsorted.size, beyond.size, many.size, one.size) == (4, 4, 130, 2)


def test_arena_swap_refuses_before_any_launch():
    from cnn_amd import capi

    lib = capi.load()
    n = 64
    buf = np.arange(2 * n, dtype=np.float32)
    a, b = buf[:n], buf[n:]
    before = buf.copy()
    for args, needle in (((None, fptr(b), n), b"null"), ((fptr(a), None, n), b"null"), ((fptr(a), fptr(b), 0), b"n=0"),
                         ((fptr(a), fptr(a), n), b"overlap"), ((fptr(a), fptr(buf[n - 1:]), n), b"overlap"),
                         ((fptr(buf[1:]), fptr(a), n), b"overlap")):
        assert lib.cnn_arena_swap(*args, None) == 1, args
        msg = lib.cnn_amd_last_error()
        assert msg.startswith(b"cnn_arena_swap") and needle in msg, (args, msg)
    assert np.array_equal(buf, before)
