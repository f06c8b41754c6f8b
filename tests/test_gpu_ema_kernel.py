"""cnn_ema_update and cnn_arena_swap (include/cnn_amd.h) on the device, through cnn_amd.capi.  Every comparison is bit-exact against the
NumPy restatement (tests/ema_ref.py; where the reference is a NaN any NaN passes); the words are compared on the device, the references
come from the host once per size."""
import numpy as np
import pytest

from tests import guarded
from tests.ema_ref import ref_ema_update
from tests.test_gpu_grad_accumulate import PAIRS, Want, make_inputs
from tests.test_gpu_optimizer import make_ranges

pytestmark = pytest.mark.gpu

# the float4 body, the <= 3-element tail and the 256-element wave chunks of the range search can each go wrong at the smallest of these
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 4099, 111267]
DECAYS = (0.0, 0.5, 0.999)


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def tables_for(n):
    """name -> averaged ranges: none, the whole buffer, three ranges cut inside float4s, and at n = 4099 seventy (the device table)"""
    out = {"none": [], "whole": [(0, n)], "three": make_ranges(50 + n, n, 3)}
    if n == 4099:
        out["seventy"] = make_ranges(51, n, 70)
        assert len(out["seventy"]) == 70
    return out


def references(n):
    """-> (ema0, p, {(decay, table name): reference output}); decay 0 ignores the table"""
    ema0, p = make_inputs(n, 9000 + n % 1000)
    refs = {}
    for name, ranges in tables_for(n).items():
        for decay in DECAYS:
            refs[(decay, name)] = ref_ema_update(ema0, p, decay, ranges)
    return ema0, p, refs


def holds_the_special_values(words):
    return (np.any(((words & 0x7F800000) == 0) & ((words & 0x007FFFFF) != 0)) and np.any(words == 0x80000000)
            and np.any((words & 0x7FFFFFFF) == 0x7F800000) and np.any((words & 0x7FFFFFFF) > 0x7F800000))


def test_inputs_test_what_they_claim():
    """(needs no device) every reference output of every size that has room for the special pairs holds a denormal, a -0.0, an infinity
    and a NaN"""
    for n in SIZES:
        if n < 3 * len(PAIRS):
            continue
        _, _, refs = references(n)
        for key, ref in refs.items():
            assert holds_the_special_values(ref.view(np.uint32)), (n, key)


def launches(rep):
    return [(k.split("|")[0], cnt) for k, (cnt, _) in rep.items()]


@pytest.mark.parametrize("n", SIZES)
def test_ema_kernel_equals_numpy_bit_for_bit(T, n):
    """all 16 element offsets of (ema, params), decay 0 / 0.5 / 0.999, every range table, ema inside a guarded allocation under both
    poisons: the result's words, the canaries, the untouched parameters, exactly one ema_ launch per call (the float4 kernel only when
    both pointers are aligned and n >= 4).  With decay 0 the destination holds the poison: it is not read."""
    from cnn_amd import capi

    ema0, p, refs = references(n)
    tables = tables_for(n)
    want = {key: Want(T, ref) for key, ref in refs.items()}
    assert np.array_equal(refs[(0.0, "whole")].view(np.uint32), p.view(np.uint32))
    ema0_dev = T.from_numpy(ema0).cuda()
    p_words = T.from_numpy(p.view(np.int32).copy()).cuda()
    keep = []
    p_ops = [guarded.operand(p, guarded.POISONS[off % 2], keep, f"params+{off}", shift_bytes=4 * off) for off in range(4)]
    problems = []
    for poison in guarded.POISONS:
        for e_off in range(4):
            ema = guarded.Scratch(4 * n, None, poison, f"ema+{e_off}", shift_bytes=4 * e_off)
            view = ema.view.view(T.float32)
            assert (view.data_ptr() % 16 == 0) == (e_off == 0)
            for p_off in range(4):
                pd = p_ops[p_off]
                assert (pd.data_ptr() % 16 == 0) == (p_off == 0)
                for decay in DECAYS:
                    for name, ranges in tables.items():
                        if decay == 0.0 and name != "whole":
                            continue
                        ema.refill()  # (decay 0: the shadow holds the poison -- it is not read)
                        if decay != 0.0:
                            view.copy_(ema0_dev)
                        T.cuda.synchronize()
                        capi.kernel_timing(1)
                        capi.ema_update(view, pd, decay, ranges)
                        rep = capi.kernel_timing_report()
                        capi.kernel_timing(0)
                        tag = f"n={n} poison={poison} ema+{e_off} params+{p_off} decay={decay} table={name}"
                        bad = want[(decay, name)].mismatches(T, view)
                        if bad:
                            problems.append(f"{tag}: {bad} element(s) differ from the reference")
                        kind = "vec" if (e_off == 0 and p_off == 0 and n >= 4) else "scalar"
                        copy = "_copy" if (decay == 0.0 or not ranges) else ""
                        if launches(rep) != [(f"ema_{kind}{copy}", 1)]:
                            problems.append(f"{tag}: launches {launches(rep)}")
                        if not ema.intact():
                            problems.append(f"{tag}: {ema.intact()}")
                        if not T.equal(pd.view(T.int32), p_words):
                            problems.append(f"{tag}: the parameters changed")
            del ema, view
    problems += guarded.check(keep)
    assert not problems, "\n  ".join(problems[:20])


@pytest.mark.parametrize("n", SIZES)
def test_three_chained_updates(T, n):
    """three updates with three parameter vectors and the warm-up's first decays = three chained reference updates"""
    from cnn_amd import capi
    from tests.ema_ref import ref_ema_decay_at

    ema0, p1 = make_inputs(n, 9100 + n % 1000)
    p2, p3 = make_inputs(n, 9200 + n % 1000)
    p3 = p3[np.random.RandomState(n).permutation(n)]
    for name, ranges in tables_for(n).items():
        ref = ema0
        for t, p in enumerate((p1, p2, p3)):
            ref = ref_ema_update(ref, p, ref_ema_decay_at(0.9, True, t), ranges)
        chained = Want(T, ref)
        for e_off, p_off in ((0, 0), (1, 0), (0, 3)):
            ema = guarded.Scratch(4 * n, None, guarded.BYTES, "ema", shift_bytes=4 * e_off)
            view = ema.view.view(T.float32)
            view.copy_(T.from_numpy(ema0).cuda())
            for t, p in enumerate((p1, p2, p3)):
                pd = guarded.operand(p, guarded.NAN, None, "params", shift_bytes=4 * p_off)
                capi.ema_update(view, pd, capi.ema_decay_at(0.9, True, t), ranges)
                T.cuda.synchronize()
            assert chained.mismatches(T, view) == 0 and ema.intact(), (n, name, e_off, p_off, str(ema.intact()))


@pytest.mark.parametrize("n", SIZES)
def test_arena_swap_exchanges_the_bits(T, n):
    """offsets 0..3 of each side, both buffers guarded: after one call the words have changed places (special values and NaN payloads
    exact), after two both are the originals; one aswap_ launch per call, the float4 kernel only when both are aligned and n >= 4"""
    from cnn_amd import capi

    a0, b0 = make_inputs(n, 9300 + n % 1000)
    a_words, b_words = T.from_numpy(a0.view(np.int32).copy()).cuda(), T.from_numpy(b0.view(np.int32).copy()).cuda()
    problems = []
    for a_off in range(4):
        for b_off in range(4):
            keep = []
            a = guarded.operand(a0, guarded.POISONS[a_off % 2], keep, f"a+{a_off}", shift_bytes=4 * a_off)
            b = guarded.operand(b0, guarded.POISONS[(b_off + 1) % 2], keep, f"b+{b_off}", shift_bytes=4 * b_off)
            for call in (1, 2):
                T.cuda.synchronize()
                capi.kernel_timing(1)
                capi.arena_swap(a, b)
                rep = capi.kernel_timing_report()
                capi.kernel_timing(0)
                tag = f"n={n} a+{a_off} b+{b_off} call {call}"
                want_a, want_b = (b_words, a_words) if call == 1 else (a_words, b_words)
                if not (T.equal(a.view(T.int32), want_a) and T.equal(b.view(T.int32), want_b)):
                    problems.append(f"{tag}: the words are not exchanged")
                kind = "vec" if (a_off == 0 and b_off == 0 and n >= 4) else "scalar"
                if launches(rep) != [(f"aswap_{kind}", 1)]:
                    problems.append(f"{tag}: launches {launches(rep)}")
            problems += guarded.check(keep)
    assert not problems, "\n  ".join(problems[:20])
