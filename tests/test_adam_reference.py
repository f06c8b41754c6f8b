"""Adam / AdamW and the global-norm clip without a GPU: the NumPy restatement of the step (tests/adam_ref.py) is the standard
algorithm, the new entry points are exported, declared and bound, and the status-returning entries check their arguments before they
launch anything."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.adam_ref import adam_host_scalars, ref_adam_step, ref_clip, ref_total_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded(n, seed):
    rs = np.random.RandomState(seed)
    p0 = rs.standard_normal(n).astype(np.float32)
    grads = [rs.standard_normal(n).astype(np.float32) for _ in range(5)]
    for g in grads:
        g[::97] = 0.0
    return p0, grads


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("decoupled", [False, True])
def test_ref_adam_step_is_torch_adam(decoupled, wd):
    """5 steps on seeded data against torch.optim.Adam / AdamW in float64 on the CPU (n = 4097, every 97th gradient exactly 0).  The
    fp32 reference rounds ~12 operations per element and step to 2^-24 relative each: orders of magnitude below rtol 1e-5 / atol
    1e-6 (the worst error measured over these cases is 0.04 of the bound).  Bit equality with torch is not asked."""
    import torch

    n, lr, betas, eps = 4097, 1e-3, (0.9, 0.999), 1e-8
    p0, grads = seeded(n, 7)
    tp = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd, amsgrad=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for step, g in enumerate(grads, start=1):
        tp.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        p, m, v = ref_adam_step(p, g, m, v, step, lr, betas[0], betas[1], eps, wd, decoupled, 1.0, [(0, n)])
        assert p.dtype == m.dtype == v.dtype == np.float32
        want = tp.detach().numpy()
        worst = max(worst, float((np.abs(p - want) / (1e-6 + 1e-5 * np.abs(want))).max()))
        assert np.allclose(p, want, rtol=1e-5, atol=1e-6), step
    state = opt.state[tp]
    assert np.allclose(m, state["exp_avg"].numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(v, state["exp_avg_sq"].numpy(), rtol=1e-5, atol=1e-6)
    print(f"decoupled={decoupled} wd={wd}: worst error {worst:.3f} of the bound")
    assert np.abs(p - p0).max() > 1e-3  # (the steps did move the parameters)


def test_ref_adam_step_special_cases():
    """weight_decay 0 ignores the ranges; decoupled decay leaves both moments independent of the parameters; elements outside the
    ranges equal the undecayed step bit for bit; a zero gradient on a zero state leaves the parameter untouched; grad_scale folds in
    front of everything"""
    rs = np.random.RandomState(3)
    n = 1000
    p, g = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    g[::97] = 0.0
    z = np.zeros(n, np.float32)
    ranges = [(10, 20), (500, n)]
    inside = np.zeros(n, bool)
    inside[10:20] = inside[500:] = True
    base = ref_adam_step(p, g, z, z, 1, 1e-3)
    for decoupled in (False, True):
        same = ref_adam_step(p, g, z, z, 1, 1e-3, weight_decay=0.0, decoupled=decoupled, decay_ranges=ranges)
        assert all(np.array_equal(a, b) for a, b in zip(base, same))
        dec = ref_adam_step(p, g, z, z, 1, 1e-3, weight_decay=0.1, decoupled=decoupled, decay_ranges=ranges)
        assert all(np.array_equal(a[~inside], b[~inside]) for a, b in zip(base, dec))
        assert not np.array_equal(dec[0][inside], base[0][inside])
    # decoupled: the moments never see the parameters
    w1 = ref_adam_step(p, g, z, z, 1, 1e-3, weight_decay=0.1, decoupled=True, decay_ranges=ranges)
    w2 = ref_adam_step(p + np.float32(3), g, z, z, 1, 1e-3, weight_decay=0.1, decoupled=True, decay_ranges=ranges)
    assert np.array_equal(w1[1], w2[1]) and np.array_equal(w1[2], w2[2]) and np.array_equal(w1[1], base[1])
    l2 = ref_adam_step(p, g, z, z, 1, 1e-3, weight_decay=0.1, decoupled=False, decay_ranges=ranges)
    assert not np.array_equal(l2[1][inside], base[1][inside])
    # g == 0 on a zero state: 0 / (0 + eps) = 0, the parameter keeps its bits (undecayed elements)
    assert np.array_equal(base[0][::97].view(np.uint32), p[::97].view(np.uint32)) and not np.any(base[1][::97]) and not np.any(base[2][::97])
    assert np.all(base[0][g != 0] != p[g != 0])
    sc = ref_adam_step(p, g, z, z, 1, 1e-3, grad_scale=0.125)
    un = ref_adam_step(p, g * np.float32(0.125), z, z, 1, 1e-3)
    assert all(np.array_equal(a, b) for a, b in zip(sc, un))
    # the host scalars: the first step's corrections are 1 - beta up to the narrowing
    om, omb1, omb2, bc2s, ss = adam_host_scalars(1, 1e-3, 0.9, 0.999, 1e-2)
    assert om == np.float32(1) - np.float32(np.float32(1e-3) * np.float32(1e-2)) and omb1 == np.float32(1) - np.float32(0.9)
    assert abs(float(bc2s) ** 2 - (1 - float(np.float32(0.999)))) < 1e-9 and abs(float(ss) - 1e-3 / (1 - float(np.float32(0.9)))) < 1e-8
    assert all(isinstance(x, np.float32) for x in (om, omb1, omb2, bc2s, ss))


def test_ref_clip_special_cases():
    rs = np.random.RandomState(4)
    g = rs.standard_normal(1000).astype(np.float32)
    norm = ref_total_norm(g)
    out, coef = ref_clip(g, norm, 0.5 * float(norm))
    assert coef < 1 and abs(float(coef) - 0.5) < 1e-6 and np.array_equal(out, g * coef)
    out, coef = ref_clip(g, norm, 2 * float(norm))
    assert coef == np.float32(1) and np.array_equal(out.view(np.uint32), g.view(np.uint32))
    out, coef = ref_clip(g, np.float32("nan"), 1.0)
    assert coef == np.float32(1) and np.array_equal(out.view(np.uint32), g.view(np.uint32))
    assert ref_total_norm(g, 0.125) == np.float32(norm * np.float32(0.125))
    assert ref_clip(g, norm, 1.0, 0.125)[1] == ref_clip(g, ref_total_norm(g, 0.125), 1.0)[1]


def test_new_symbols_are_exported_declared_and_bound():
    """libcnn_amd.so / libcnn_amd_host.so export the new entry points, the headers declare them, the ctypes tables bind them"""
    from cnn_amd import capi, hostapi

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}

    have = exported(capi.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cnn_amd.h")).read(), flags=re.S)
    for name in ("cnn_adam_update", "cnn_clip_grad_norm", "cnn_clip_grad_norm_workspace_bytes"):
        assert name in have and hasattr(capi.load(), name) and name in capi.SIGNATURES, name
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", hdr), name
    host_syms = ["cnnh_net_set_adam", "cnnh_net_adam_m_device", "cnnh_net_adam_v_device", "cnnh_net_get_adam_state", "cnnh_net_set_grad_clip",
                 "cnnh_net_last_grad_norm"]
    host_have = exported(hostapi.LIB_PATH)
    for name in host_syms:
        assert name in host_have and name in hostapi.SIGNATURES, name
    m = re.search(r"typedef\s+struct\s+cnn_adam_options\s*\{(.*?)\}\s*cnn_adam_options\s*;", hdr, flags=re.S)
    fields = ["lr", "beta1", "beta2", "eps", "weight_decay", "decoupled", "step"]
    assert m and re.findall(r"\b(lr|beta1|beta2|eps|weight_decay|decoupled|step)\b", m.group(1)) == fields
    assert [n for n, _ in capi.AdamOptions._fields_] == fields and C.sizeof(capi.AdamOptions) == 32
    assert int(re.search(r"#define\s+CNN_CLIP_MAX_BLOCKS\s+(\d+)", hdr).group(1)) == capi.CLIP_MAX_BLOCKS
    assert capi.load().cnn_amd_abi_version() == 2
    arch = open(os.path.join(ROOT, "cnn_amd", "host", "include", "architectures.h")).read()
    for decl in ("void set_adam(", "void set_grad_clip(", "data_type last_grad_norm(", "adam_m_device()", "adam_v_device()", "adam_step()"):
        assert decl in arch, decl
    for meth in ("set_adam", "get_adam_state", "set_grad_clip", "last_grad_norm"):
        assert hasattr(hostapi.HostNet, meth), meth


@pytest.mark.parametrize("name", ["cnn_adam_update", "cnn_clip_grad_norm"])
def test_null_arguments_of_the_new_entries_in_a_child_process(name):
    """tests/sweeps/null_args.py on each new status-returning entry alone: all pointers NULL, once with every size zero (no crash),
    once with non-zero sizes (a non-zero status and a message) -- in a child process, so that a dereference would show as a signal"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweeps", "null_args.py"), name], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-2000:])
    assert r.stdout.startswith("rc 1 ") and "null" in r.stdout, r.stdout


def test_adam_argument_checks_come_before_any_launch():
    """every refusal below is decided on the host (CNN_AMD_E_BADARG = 1 with a message); the pointers that stand for device memory
    are never dereferenced"""
    from cnn_amd import capi

    lib = capi.load()
    fake = C.c_void_p(0x1000)
    n = 100

    def call(opt, ranges=(), dev=None, ptrs=(fake, fake, fake, fake), n_=n, n_ranges=None):
        tab = np.asarray(ranges, np.uint32).reshape(-1)
        nr = tab.size // 2 if n_ranges is None else n_ranges
        return lib.cnn_adam_update(*ptrs, n_, C.byref(opt) if opt is not None else None, 1.0,
                                   tab.ctypes.data_as(C.c_void_p) if tab.size else None, dev, nr, None, None)

    def opts(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, decoupled=0, step=1):
        return capi.AdamOptions(lr, beta1, beta2, eps, wd, decoupled, step)

    assert call(opts(), n_=0) == 0  # nothing to do
    assert call(None) == 1 and b"null" in lib.cnn_amd_last_error()
    for k in range(4):
        ptrs = [fake] * 4
        ptrs[k] = None
        assert call(opts(), ptrs=tuple(ptrs)) == 1 and b"null" in lib.cnn_amd_last_error(), k
    for bad in (opts(beta1=1.0), opts(beta1=-0.1), opts(beta2=1.0), opts(beta2=-0.5), opts(beta1=float("nan"))):
        assert call(bad) == 1 and b"beta" in lib.cnn_amd_last_error()
    for bad in (opts(eps=0.0), opts(eps=-1e-8), opts(eps=float("nan"))):
        assert call(bad) == 1 and b"eps" in lib.cnn_amd_last_error()
    assert call(opts(wd=-1e-2)) == 1 and b"weight_decay" in lib.cnn_amd_last_error()
    assert call(opts(wd=float("nan"))) == 1
    assert call(opts(step=0)) == 1 and b"step" in lib.cnn_amd_last_error()
    for bad in ([(10, 10)], [(20, 10)], [(0, 50), (40, 60)], [(50, 60), (0, 10)], [(90, 101)]):
        assert call(opts(), bad) == 1 and b"range" in lib.cnn_amd_last_error(), bad
    assert call(opts(), n_ranges=3) == 1  # a count without a table
    many = [(2 * i, 2 * i + 1) for i in range(capi.SGD_INLINE_RANGES + 1)]
    assert call(opts(), many, n_=1000) == 1 and b"decay_ranges_dev" in lib.cnn_amd_last_error()
    assert call(opts(), n_=1 << 32) == 1 and b"32-bit" in lib.cnn_amd_last_error()


def test_clip_argument_checks_come_before_any_launch():
    from cnn_amd import capi

    lib = capi.load()
    fake = C.c_void_p(0x1000)
    n = 1000
    need = lib.cnn_clip_grad_norm_workspace_bytes(n)
    assert need == 8 * 4  # ceil(1000 / 256) workgroups
    assert lib.cnn_clip_grad_norm_workspace_bytes(1) == 8
    assert lib.cnn_clip_grad_norm_workspace_bytes(1 << 30) == 8 * capi.CLIP_MAX_BLOCKS

    def call(g=fake, n_=n, max_norm=1.0, ws=fake, ws_bytes=need, stats=fake):
        return lib.cnn_clip_grad_norm(g, n_, max_norm, 1.0, ws, ws_bytes, stats, None)

    for kw in (dict(g=None), dict(ws=None), dict(stats=None)):
        assert call(**kw) == 1 and b"null" in lib.cnn_amd_last_error(), kw
    assert call(n_=0) == 1 and b"n=0" in lib.cnn_amd_last_error()
    for bad in (0.0, -1.0, float("nan")):
        assert call(max_norm=bad) == 1 and b"max_norm" in lib.cnn_amd_last_error(), bad
    assert call(ws_bytes=need - 8) == 1 and (b"needs %d" % need) in lib.cnn_amd_last_error()
