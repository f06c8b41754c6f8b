"""The optimizer without a GPU: the NumPy restatement of the step (tests/optim_ref.py) is the standard algorithm, the new entry
points are exported, declared and bound, and the status-returning entry checks its arguments before it launches anything."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.optim_ref import decay_ranges_of, ref_sgd_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("momentum,wd,nesterov", [(0.9, 0.0, False), (0.9, 5e-4, False), (0.9, 5e-4, True)])
def test_ref_sgd_step_is_torch_sgd(momentum, wd, nesterov):
    """5 steps on seeded data against torch.optim.SGD on the CPU.  A few ulp (2^-24 relative) per operation over 5 steps is several
    orders of magnitude below rtol 1e-5 / atol 1e-6; torch may contract p + (-lr) * buf, so bit equality with it is not asked."""
    import torch

    n, lr = 4099, 0.05
    rs = np.random.RandomState(7)
    p0 = rs.standard_normal(n).astype(np.float32)
    grads = [rs.standard_normal(n).astype(np.float32) for _ in range(5)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov, dampening=0)
    p, v = p0.copy(), np.zeros(n, np.float32)
    for g in grads:
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, v = ref_sgd_step(p, g, v, lr, momentum, wd, nesterov, decay_ranges=[(0, n)])
        assert p.dtype == np.float32 and v.dtype == np.float32
        assert np.allclose(p, tp.detach().numpy(), rtol=1e-5, atol=1e-6)
    buf = opt.state[tp]["momentum_buffer"].numpy()
    assert np.allclose(v, buf, rtol=1e-5, atol=1e-6)
    assert np.abs(p - p0).max() > 0.1  # (the steps did move the parameters)


def test_ref_sgd_step_special_cases():
    """momentum 0 / weight decay 0 is the reference's w -= lr * g (two roundings); decay stays inside its ranges; grad_scale folds in
    front of everything; momentum 0 hands the velocity back untouched"""
    rs = np.random.RandomState(3)
    n = 1000
    p, g = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    lr = np.float32(0.01)
    sentinel = np.full(n, 7.5, np.float32)
    p1, v1 = ref_sgd_step(p, g, sentinel, lr)
    assert v1 is sentinel and np.array_equal(p1, p - lr * g)
    p2, _ = ref_sgd_step(p, g, None, lr, 0.0, 0.1, decay_ranges=[(10, 20), (500, n)])
    inside = np.zeros(n, bool)
    inside[10:20] = inside[500:] = True
    assert np.array_equal(p2[~inside], p1[~inside]) and not np.any(p2[inside] == p1[inside])
    assert np.array_equal(p2[inside], (p - lr * (g + np.float32(0.1) * p))[inside])
    p3, _ = ref_sgd_step(p, g, None, lr, grad_scale=0.125)
    assert np.array_equal(p3, p - lr * (g * np.float32(0.125)))
    p4, v4 = ref_sgd_step(p, g, np.zeros(n, np.float32), lr, 0.9, nesterov=True)
    assert np.array_equal(v4, g) and np.array_equal(p4, p - lr * (g + np.float32(0.9) * g))  # (first step from a zero velocity)


def test_decay_policy_of_a_layout():
    """weights only by default; biases and gamma / beta on request (neighbouring ranges merge); never the moving statistics"""
    from cnn_amd import stacks as S

    layout = S.walk(S.alexnet(3, batch_norm=True))
    plain = decay_ranges_of(layout)
    assert plain[0] == (0, 16 * 27) and len(plain) == 5 and plain[-1][1] == sum(e["params"] for e in layout) - 3
    wide = decay_ranges_of(layout, True)
    assert wide[0] == (0, 16 * 27 + 16 + 32)  # conv_layer_1's weights + bias, bn_layer_1's gamma + beta
    assert wide[1][0] == wide[0][1] + 32      # ... and its moving statistics stay out
    assert wide[-1][1] == sum(e["params"] for e in layout)


def test_new_symbols_are_exported_declared_and_bound():
    """libcnn_amd.so / libcnn_amd_host.so export the optimizer's entry points, the headers declare them, the ctypes tables bind them"""
    from cnn_amd import capi, hostapi

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}

    assert "cnn_sgd_momentum_update" in exported(capi.LIB_PATH)
    assert hasattr(capi.load(), "cnn_sgd_momentum_update") and "cnn_sgd_momentum_update" in capi.SIGNATURES
    host_syms = ["cnnh_net_set_optimizer", "cnnh_net_save_optimizer_state", "cnnh_net_load_optimizer_state", "cnnh_net_velocity_device",
                 "cnnh_net_get_velocity", "cnnh_net_forward_backward_device_loss"]
    have = exported(hostapi.LIB_PATH)
    for name in host_syms:
        assert name in have, name
        assert name in hostapi.SIGNATURES, name
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cnn_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+cnn_sgd_momentum_update\s*\(", hdr)
    m = re.search(r"typedef\s+struct\s+cnn_sgd_options\s*\{(.*?)\}\s*cnn_sgd_options\s*;", hdr, flags=re.S)
    assert m and [w for w in re.findall(r"\b(lr|momentum|weight_decay|nesterov)\b", m.group(1))] == ["lr", "momentum", "weight_decay", "nesterov"]
    assert [n for n, _ in capi.SgdOptions._fields_] == ["lr", "momentum", "weight_decay", "nesterov"] and C.sizeof(capi.SgdOptions) == 16
    assert int(re.search(r"#define\s+CNN_SGD_INLINE_RANGES\s+(\d+)", hdr).group(1)) == capi.SGD_INLINE_RANGES
    arch = open(os.path.join(ROOT, "cnn_amd", "host", "include", "architectures.h")).read()
    for decl in ("void set_optimizer(", "int save_optimizer_state(", "int load_optimizer_state(", "velocity_device()", "decay_ranges("):
        assert decl in arch, decl


def test_null_arguments_of_the_new_entry_in_a_child_process():
    """tests/sweeps/null_args.py on cnn_sgd_momentum_update alone: all pointers NULL, once with every size zero (no crash), once with
    non-zero sizes (a non-zero status and a message) -- in a child process, so that a dereference would show as a signal"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweeps", "null_args.py"), "cnn_sgd_momentum_update"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-2000:])
    assert r.stdout.startswith("rc 1 ") and "null" in r.stdout, r.stdout


def test_argument_checks_come_before_any_launch():
    """every refusal below is decided on the host (CNN_AMD_E_BADARG = 1 with a message); the pointers that stand for device memory
    are never dereferenced"""
    from cnn_amd import capi

    lib = capi.load()
    fake = C.c_void_p(0x1000)
    n = 100

    def call(opt, ranges, dev=None, velocity=fake, n_=n, n_ranges=None):
        tab = np.asarray(ranges, np.uint32).reshape(-1)
        nr = tab.size // 2 if n_ranges is None else n_ranges
        return lib.cnn_sgd_momentum_update(fake, fake, velocity, n_, C.byref(opt) if opt is not None else None, 1.0,
                                           tab.ctypes.data_as(C.c_void_p) if tab.size else None, dev, nr, None, None)

    ok = capi.SgdOptions(0.1, 0.9, 5e-4, 0)
    assert call(ok, [], n_=0) == 0  # nothing to do
    assert call(None, []) == 1 and b"null" in lib.cnn_amd_last_error()
    assert call(ok, [], velocity=None) == 1 and b"velocity" in lib.cnn_amd_last_error()
    assert call(capi.SgdOptions(0.1, -0.5, 0.0, 0), []) == 1 and b"momentum" in lib.cnn_amd_last_error()
    assert call(capi.SgdOptions(0.1, 0.9, float("nan"), 0), []) == 1
    for bad in ([(10, 10)], [(20, 10)], [(0, 50), (40, 60)], [(50, 60), (0, 10)], [(90, 101)]):
        assert call(ok, bad) == 1 and b"range" in lib.cnn_amd_last_error(), bad
    assert call(ok, [], n_ranges=3) == 1  # a count without a table
    many = [(2 * i, 2 * i + 1) for i in range(capi.SGD_INLINE_RANGES + 1)]
    assert call(ok, many, n_=1000) == 1 and b"decay_ranges_dev" in lib.cnn_amd_last_error()
    assert call(ok, [], n_=1 << 32) == 1 and b"32-bit" in lib.cnn_amd_last_error()
