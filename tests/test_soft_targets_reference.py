"""Soft targets without a device: the NumPy restatement (tests/soft_target_ref.py) against CPU torch, every refusal of the new
C ABI entries (argument checks come before any launch), cnn_cutmix_lambda, the host-side sampler hostapi.mix_params, and the host
library's new exports."""
import ctypes as C

import numpy as np
import pytest

from tests.soft_target_ref import (MIX_CUTMIX, MIX_MIXUP, PAIR_FLIP, PAIR_NONE, PAIR_ROLL, ref_batch_mix, ref_cutmix_lambda, ref_partner,
                                   ref_soft_loss, ref_soft_targets)

B = 7
EPS32 = 2.0 ** -24


def _case(classes, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((B, classes)) * 2).astype(np.float32), rs.randint(0, classes, size=B).astype(np.int32)


@pytest.mark.parametrize("classes", [3, 10])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [0.3, 1.0])
def test_restatement_equals_torch_cross_entropy(classes, eps, lam):
    """mean_b(-sum_j t_j log_softmax_j) in float64 against F.cross_entropy(label_smoothing=eps), mixed: lam * CE(a) + (1 - lam) * CE(b).
    eps = 0 and lam = 1: exactly one-hot targets, 1e-12 relative.  Otherwise a target value carries the roundings of the four fp32
    operations that build it (the division, two products, one sum): 4 * 2^-24 relative to sum |t_j log p_j|."""
    import torch
    import torch.nn.functional as Fn

    logits, labels = _case(classes, 10 * classes + int(eps * 10))
    t = ref_soft_targets(labels, classes, eps, lam, PAIR_FLIP)
    got, _, scale = ref_soft_loss(logits, t)
    z = torch.from_numpy(logits).double()
    la = torch.from_numpy(labels).long()
    lb = la[torch.from_numpy(ref_partner(B, PAIR_FLIP).copy())]
    lam32 = float(np.float32(lam))
    want = float(lam32 * Fn.cross_entropy(z, la, label_smoothing=eps) + (1.0 - lam32) * Fn.cross_entropy(z, lb, label_smoothing=eps))
    if eps == 0.0 and lam == 1.0:
        assert np.array_equal(t, np.eye(classes, dtype=np.float32)[labels])
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    else:
        bound = 4 * EPS32 * scale / B
        print(f"classes={classes} eps={eps} lam={lam}: |diff| {abs(got - want):.3e}, bound {bound:.3e}")
        assert abs(got - want) <= bound, (got, want, bound)


@pytest.mark.parametrize("classes", [3, 10])
def test_restatement_delta_is_the_gradient(classes):
    """autograd of sum_b(-sum_j t_j log_softmax_j) is p * sum_j t_j - t; the restatement's delta is p - t, so the two differ by exactly
    p * (sum_j t_j - 1), the rounding of the target row's sum"""
    import torch

    logits, labels = _case(classes, 77)
    t = ref_soft_targets(labels, classes, 0.1, 0.3, PAIR_ROLL, 2)
    _, delta, _ = ref_soft_loss(logits, t)
    z = torch.from_numpy(logits).double().requires_grad_(True)
    td = torch.from_numpy(t).double()
    (-(td * torch.log_softmax(z, dim=1)).sum()).backward()
    p = torch.softmax(z.detach(), dim=1).numpy()
    row = t.astype(np.float64).sum(axis=1, keepdims=True) - 1.0
    assert np.all(np.abs(row) <= classes * EPS32)
    assert np.allclose(z.grad.numpy() - delta, p * row, rtol=0, atol=1e-15)


def test_targets_restatement_properties():
    labels = np.array([0, 2, 1, -1, 3], np.int32)
    hard = ref_soft_targets(labels, 3)
    assert hard.dtype == np.float32 and np.array_equal(hard[:3], np.eye(3, dtype=np.float32)[[0, 2, 1]])
    assert not hard[3].any() and not hard[4].any()  # a label outside [0, classes) matches no column
    s = ref_soft_targets(labels, 3, 0.1)
    assert s[0, 0] == (np.float32(1) - np.float32(0.1)) + np.float32(0.1) / np.float32(3) and s[0, 1] == np.float32(0.1) / np.float32(3)
    assert np.array_equal(ref_soft_targets(labels, 3, 0.1, 1.0, PAIR_FLIP), s)  # lam == 1: no partner
    assert np.array_equal(ref_soft_targets(labels, 3, 0.1, 0.0, PAIR_ROLL, 1), s[ref_partner(5, PAIR_ROLL, 1)])
    assert list(ref_partner(5, PAIR_FLIP)) == [4, 3, 2, 1, 0] and list(ref_partner(5, PAIR_ROLL, 4)) == [4, 0, 1, 2, 3]


def test_mix_restatement_properties():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((5, 3, 7, 9)).astype(np.float32)
    x.view(np.uint32)[0, 0, 0, :4] = [0x80000000, 0x7FC01234, 0x00000001, 0xFF800000]  # -0.0, a NaN payload, a denormal, -inf
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert same(ref_batch_mix(x, MIX_MIXUP, 1.0, PAIR_FLIP), x) and same(ref_batch_mix(x, MIX_CUTMIX, 0.5, PAIR_NONE, box=(0, 7, 0, 9)), x)
    assert same(ref_batch_mix(x, MIX_CUTMIX, 0.0, PAIR_FLIP, box=(2, 2, 0, 9)), x)
    full = ref_batch_mix(x, MIX_CUTMIX, 0.0, PAIR_FLIP, box=(0, 7, 0, 9))
    assert same(full, x[::-1].copy())
    m = ref_batch_mix(x, MIX_MIXUP, 0.3, PAIR_ROLL, 1)
    want = np.float32(0.3) * x[1] + (np.float32(1) - np.float32(0.3)) * x[2]
    assert same(m[1], want.astype(np.float32))


def _lib():
    from cnn_amd import capi

    return capi, capi.load()


def test_every_refusal_is_badarg_with_a_message():
    """nothing here reaches a launch: the pointers are small non-null integers that are never dereferenced"""
    capi, lib = _lib()
    p, q = C.c_void_p(0x1000), C.c_void_p(0x100000)
    nan = float("nan")

    def refused(rc, word):
        assert rc == 1, (rc, word)  # CNN_AMD_E_BADARG
        msg = lib.cnn_amd_last_error().decode()
        assert word in msg, (word, msg)

    st = lib.cnn_soft_targets
    refused(st(None, q, 4, 3, 0.1, 0.5, 0, 0, None), "null")
    refused(st(p, None, 4, 3, 0.1, 0.5, 0, 0, None), "null")
    refused(st(p, q, 0, 3, 0.1, 0.5, 0, 0, None), "B=0")
    refused(st(p, q, 4, 0, 0.1, 0.5, 0, 0, None), "classes=0")
    for s in (-0.1, 1.0, nan):
        refused(st(p, q, 4, 3, s, 0.5, 0, 0, None), "smoothing")
    for lam in (-0.1, 1.5, nan):
        refused(st(p, q, 4, 3, 0.1, lam, 0, 0, None), "lam")
    refused(st(p, q, 4, 3, 0.1, 0.5, 3, 0, None), "pair_rule")
    for shift in (0, 4, -1):
        refused(st(p, q, 4, 3, 0.1, 0.5, capi.PAIR_ROLL, shift, None), "shift")

    bm = lib.cnn_batch_mix
    ok = dict(mode=capi.MIX_MIXUP, lam=0.5, pair_rule=capi.PAIR_FLIP, pair_shift=0, y0=0, y1=2, x0=0, x1=2)
    call = lambda src=p, dst=q, dims=(4, 3, 8, 8), **kw: bm(C.byref(capi.MixDesc(**{**ok, **kw})), src, dst, *dims, None)
    refused(bm(None, p, q, 4, 3, 8, 8, None), "null")
    refused(call(src=None), "null")
    refused(call(dst=None), "null")
    for dims in ((0, 3, 8, 8), (4, 0, 8, 8), (4, 3, 0, 8), (4, 3, 8, 0)):
        refused(call(dims=dims), "B=")
    refused(call(mode=0), "mode")
    refused(call(mode=3), "mode")
    refused(call(pair_rule=7), "pair_rule")
    refused(call(pair_rule=capi.PAIR_ROLL, pair_shift=4), "shift")
    for lam in (-0.5, 1.25, nan):
        refused(call(lam=lam), "lam")
    for box in (dict(y0=-1), dict(y0=3, y1=2), dict(y1=9), dict(x0=-1), dict(x0=3, x1=2), dict(x1=9)):
        refused(call(mode=capi.MIX_CUTMIX, **box), "box")
    refused(call(dst=p), "overlap")
    refused(call(dst=C.c_void_p(0x1000 + 4 * (4 * 3 * 8 * 8 - 1))), "overlap")

    for fn, n_ptr in ((lib.cnn_softmax_xent_soft, 5), (lib.cnn_linear_forward_softmax_xent_soft, 8), (lib.cnn_linear_forward_softmax_xent_soft_dx, 9)):
        ints = {5: (4, 3), 8: (4, 16, 3), 9: (1, 4, 16, 3)}[n_ptr]
        refused(fn(*([None] * n_ptr), *ints, None), "null")
    refused(lib.cnn_softmax_xent_soft(p, p, p, p, p, 0, 3, None), "B=0")
    refused(lib.cnn_linear_forward_softmax_xent_soft(*([p] * 8), 4, 16, 9, None), "out=9")
    refused(lib.cnn_linear_forward_softmax_xent_soft_dx(*([p] * 9), 0, 4, 16, 9, None), "out=9")


def test_cutmix_lambda_on_a_full_an_empty_and_a_one_pixel_box():
    capi, _ = _lib()
    assert capi.cutmix_lambda(224, 224, 0, 224, 0, 224) == 0.0
    assert capi.cutmix_lambda(224, 224, 17, 17, 0, 224) == 1.0 and capi.cutmix_lambda(224, 224, 0, 224, 5, 5) == 1.0
    assert np.float32(capi.cutmix_lambda(7, 9, 6, 7, 8, 9)) == np.float32(1.0 - 1.0 / 63.0)
    for args in ((224, 224, 56, 168, 56, 168), (7, 9, 1, 4, 2, 7)):
        assert np.float32(capi.cutmix_lambda(*args)) == ref_cutmix_lambda(*args)


def test_mix_params_sampler():
    from cnn_amd import capi, hostapi

    fields = lambda d: tuple(getattr(d, n) for n, _ in capi.MixDesc._fields_)
    a = [fields(hostapi.mix_params(np.random.default_rng(5), 224, 200)) for _ in range(3)]
    assert a[0] == a[1] == a[2]  # (seeded: reproducible)
    rng = np.random.default_rng(11)
    modes = set()
    for _ in range(200):
        d = hostapi.mix_params(rng, 37, 53)
        modes.add(d.mode)
        assert 0.0 <= d.lam <= 1.0 and d.pair_rule == capi.PAIR_FLIP
        if d.mode == capi.MIX_CUTMIX:
            assert 0 <= d.y0 <= d.y1 <= 37 and 0 <= d.x0 <= d.x1 <= 53
            assert np.float32(d.lam) == np.float32(capi.cutmix_lambda(37, 53, d.y0, d.y1, d.x0, d.x1))
    assert modes == {capi.MIX_MIXUP, capi.MIX_CUTMIX}
    assert {hostapi.mix_params(rng, 37, 53, switch_prob=0.0).mode for _ in range(50)} == {capi.MIX_MIXUP}
    assert {hostapi.mix_params(rng, 37, 53, switch_prob=1.0).mode for _ in range(50)} == {capi.MIX_CUTMIX}
    with pytest.raises(capi.CnnAmdError):
        hostapi.mix_params(rng, 8, 8, mixup_alpha=0.0, cutmix_alpha=0.0)


def test_host_library_exports_the_soft_target_entries():
    from cnn_amd import capi, hostapi

    lib = hostapi.load()
    for name in ("cnnh_net_set_label_smoothing", "cnnh_net_train_step_mixed", "cnnh_net_train_step_soft", "cnnh_net_get_targets"):
        assert name in hostapi.SIGNATURES and hasattr(lib, name), name
    for name in ("cnn_soft_targets", "cnn_batch_mix", "cnn_cutmix_lambda", "cnn_softmax_xent_soft", "cnn_linear_forward_softmax_xent_soft",
                 "cnn_linear_forward_softmax_xent_soft_dx"):
        assert name in capi.SIGNATURES, name
    assert C.sizeof(capi.MixDesc) == 32
    for name in ("set_label_smoothing", "train_step_mixed", "train_step_soft", "last_targets"):
        assert callable(getattr(hostapi.HostNet, name))
