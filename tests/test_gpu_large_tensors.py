"""Tensors at the 32-bit index limits of the kernel families: every fast family declines, switches variant or
refuses at 2^29 elements (32-bit BYTE offsets), 2^31 elements (int element indices) or 2^32 elements (the implicit GEMM's DMA descriptor).
Each case runs one batch just UNDER its documented limit -- the family's kernel with its highest offsets -- and one just OVER it -- the
kernel that takes over, at a size nothing else in the suite reaches.

Rules of every case (tests/large.py):
  * the batch comes from the documented limit (batch_under), never from the library's plan / *_supported functions;
  * the launch log (capi.kernel_timing) pins which side ran: the family's name appears under the limit and not over it; the kernel that
    took over is in the assertion message and in the `LARGE` report line;
  * the oracle judges slices at the project tolerance (tests.util.REL_TOL through assert_close): forward and data gradient on samples
    0, 1, B//2, B-2, B-1 (per-sample independent passes; the last samples carry the highest offsets); the weight gradient through a delta
    that is zero except on samples 0, B//2, B-1 (= the oracle's gradient of those samples x 3/B), then exact linearity with every sample
    live (dy * 2 doubles every bit pattern's exponent only);
  * outputs are pre-filled with 7.0; where a ReLU' form exists, dxm == where(relu_in <= 0, 0, dx) over the WHOLE tensor, on the device,
    in sample chunks; no large tensor is ever copied to the host;
  * the footprint is computed before anything is allocated; the case skips (with both numbers) only if the device has less than
    footprint + 4 GiB free, and hands its memory back at the end.

Inputs are those of the existing full-size tests (tests/test_gpu_stacks.py): x uniform in [-0.4, 0.6), He-scaled weights, dy in +-1.

Every case prints one `LARGE` line (pytest -rA / -s): batch, computed footprint, measured peak device memory, seconds, and the kernels
that ran in each pass.  Computed footprints: tier A <= 14 GiB per case, tier B <= 45 GiB, tier C 35 GiB.
"""
import time

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import large
from tests.large import GIB, batch_under
from tests.util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu

L29, L31, L32 = 1 << 29, 1 << 31, 1 << 32


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    assert capi.load().cnn_amd_device_arch().decode() == "gfx950"
    return torch


def has(*parts):
    """predicate on a kernel name: starts with parts[0] and contains every further part"""
    return lambda n: n.startswith(parts[0]) and all(p in n for p in parts[1:])


# One row per family and limit.  geom = (Ci, H, W, Co, k, s, pad); `per` = elements per sample of the tensor the limit is about;
# fwd / dgrad / wgrad: (predicate of the family's kernel name, what the log shows OVER the limit: "absent" | "present"), or None = the pass
# is not part of the row.  "present" over the limit: the guard that binds at this batch belongs to another pass of the row (the pass runs
# and is checked on both sides all the same).  `log`: passes that are run and held to the oracle with their kernel only recorded.
def _elems(c, h, w):
    return c * h * w


CONV_ROWS_TABLE = {
    # ---- tier A: 2^29 elements (32-bit byte offsets) ----
    "A-conv_rows-112": dict(tier="A", geom=(64, 112, 112, 64, 3, 1, 1), per=_elems(64, 112, 112), limit=L29, expect=(668, 669),
                            fwd=(has("conv_rows<"), "absent"), dgrad=(has("conv_rows<"), "absent")),
    "A-conv_rows-28": dict(tier="A", geom=(128, 28, 28, 128, 3, 1, 1), per=_elems(128, 28, 28), limit=L29, expect=(5349, 5350),
                           fwd=(has("conv_rows<"), "absent"), dgrad=(has("conv_rows<"), "absent")),
    # (pad 0: the data gradient reads dy, 64 x 50 x 50 per sample -- below 2^29 on both sides, it stays on the family)
    "A-conv_rows_any+wgrad_sp_any": dict(tier="A", geom=(64, 52, 52, 64, 3, 1, 0), per=_elems(64, 52, 52), limit=L29, expect=(3102, 3103),
                                         fwd=(has("conv_rows_any<"), "absent"), dgrad=(has("conv_rows_any<"), "present"),
                                         wgrad=(has("wgrad_sp_any<"), "absent")),
    # (the 56-wide data gradient is not a default instance of conv_rows_s2: it runs on the m16 variant of conv_dgrad_rd, same limit)
    "A-conv_s2+wgrad_sp2": dict(tier="A", geom=(64, 56, 56, 128, 3, 2, 1), per=_elems(64, 56, 56), limit=L29, expect=(2674, 2675),
                                fwd=(has("conv_s2<", "/fwd"), "absent"), dgrad=(has("conv_dgrad_rd<", "m16"), "absent"), wgrad=(has("wgrad_sp2<"), "absent")),
    "A-wgrad_sp": dict(tier="A", geom=(64, 56, 56, 64, 3, 1, 1), per=_elems(64, 56, 56), limit=L29, expect=(2674, 2675),
                       fwd=(has("conv_rows<"), "absent"), dgrad=(has("conv_rows<"), "absent"), wgrad=(has("wgrad_sp<"), "absent")),
    # (reference layer 2: the m16 variants of the register-direct kernels address x through a buffer descriptor; the weight gradient's
    #  families -- wgrad_os / wgrad_rd -- index in 64 bits below 2^30 units: recorded, held to the oracle on both sides)
    "A-rd-m16": dict(tier="A", geom=(16, 111, 111, 32, 3, 2, 0), per=_elems(16, 111, 111), limit=L29, expect=(2723, 2724),
                     fwd=(has("conv_fwd_rd<", "m16"), "absent"), dgrad=(has("conv_dgrad_rd<", "m16"), "absent"), log=("wgrad",)),
    # (7x7 stem: the limit is on dy, 64 x 112 x 112 per sample)
    "A-stem-dgrad-thin": dict(tier="A", geom=(3, 224, 224, 64, 7, 2, 3), per=_elems(64, 112, 112), limit=L29, expect=(668, 669),
                              dgrad=(has("conv_dgrad_thin"), "absent")),
    # ---- tier B: 2^31 elements (int element indices) ----
    # (Co = 32 without the m16 variant: the data gradient is not on conv_dgrad_rd on either side -- recorded; wgrad_rd switches to its
    #  guarded windows inside the same kernel -- recorded)
    "B-rd-elements": dict(tier="B", geom=(16, 111, 111, 32, 3, 2, 0), per=_elems(16, 111, 111), limit=L31, expect=(10893, 10894),
                          fwd=(has("conv_fwd_rd<"), "absent"), log=("dgrad", "wgrad"), relu=False),
    # (the OUTPUT guard: x stays below 2^29; the data gradient reads the 2^31-element dy and is elsewhere on both sides -- recorded)
    "B-conv_rows-output": dict(tier="B", geom=(16, 112, 112, 128, 3, 1, 1), per=_elems(128, 112, 112), limit=L31, expect=(1337, 1338),
                               fwd=(has("conv_rows<"), "absent"), log=("dgrad",), relu=False),
    "B-conv_stem": dict(tier="B", geom=(3, 224, 224, 64, 7, 2, 3), per=_elems(64, 112, 112), limit=L31, expect=(2674, 2675),
                        fwd=(has("conv_stem_fwd<"), "absent"), log=("wgrad",)),
    # ---- tier C: 2^32 elements: the in-kernel B*C*XH*XW < 2^32 descriptor switch of igemm_dma_kernel (same kernel name on both sides) ----
    "C-igemm-dma": dict(tier="C", geom=(64, 112, 112, 64, 3, 1, 1), per=_elems(64, 112, 112), limit=L32, expect=(5349, 5350),
                        fwd=(has("igemm_dma_kernel<"), "present"), dgrad=(has("igemm_dma_kernel<"), "present"), relu=False, lean=True,
                        sel=lambda B: [0, B - 1]),
}


def _check_log(row_id, side, what, spec, names, refused):
    pred, over = spec
    hit = [n for n in names if pred(n)]
    if side == "under":
        assert not refused and hit, f"{row_id} {what}: the family's kernel did not run UNDER its limit; launched: {names} {refused or ''}"
    elif over == "absent":
        assert not hit, f"{row_id} {what}: the family's kernel {hit} ran OVER its limit; launched: {names}"
    else:
        assert refused or hit, f"{row_id} {what}: launched: {names}"


@pytest.mark.parametrize("side", ["under", "over"])
@pytest.mark.parametrize("row_id", list(CONV_ROWS_TABLE), ids=lambda r: r)
def test_conv_family_on_both_sides_of_its_limit(T, row_id, side):
    from cnn_amd import capi

    row = CONV_ROWS_TABLE[row_id]
    Ci, H, W, Co, k, s, pad = row["geom"]
    under = batch_under(row["per"], row["limit"])
    assert (under, under + 1) == row["expect"], (under, row["expect"])  # (the numbers of DESIGN.md section 11)
    B = under if side == "under" else under + 1
    assert (B * row["per"] < row["limit"]) == (side == "under")
    t0 = time.time()
    passes = {p: row.get(p) for p in ("fwd", "dgrad", "wgrad")}
    logged = row.get("log", ())
    run = {p: passes[p] is not None or p in logged for p in passes}
    relu = row.get("relu", True) and run["dgrad"]
    lean = row.get("lean", False)
    Ho, Wo = capi.conv_out_dim(H, k, s, pad), capi.conv_out_dim(W, k, s, pad)
    nx1, ny1 = Ci * H * W, Co * Ho * Wo
    nx, ny = B * nx1, B * ny1
    desc = capi.ConvDesc(B, Ci, H, W, Co, k, s, pad)
    import ctypes

    ws_bytes = int(capi.load().cnn_conv2d_workspace_bytes(ctypes.byref(desc)))
    assert ws_bytes > 0, capi.load().cnn_amd_last_error()
    # tensors alive at the peak: x, y, dy (+ dx, + relu_in and dxm); lean rows hold (x, y), then (dy, dx); + the chunk temporaries
    if lean:
        n_float = max(nx + ny, ny + nx)
    else:
        n_float = nx + ny * (1 if not (run["dgrad"] or run["wgrad"]) else 2) + (nx if run["dgrad"] else 0) + (2 * nx if relu else 0)
    footprint = 4 * n_float + ws_bytes + 4 * (1 << 27) * 4
    large.require_memory(T, footprint, row_id)

    g = T.Generator(device="cuda").manual_seed(23)
    w = T.randn((Co, Ci, k, k), generator=g, device="cuda") * float(np.sqrt(2.0 / (Ci * k * k)))
    b = T.randn((Co,), generator=g, device="cuda") * 0.1
    wn, bn_ = w.cpu().numpy(), b.cpu().numpy()
    conv = capi.Conv2d(B, Ci, H, W, Co, k, s, pad)
    sel = row["sel"](B) if "sel" in row else [0, 1, B // 2, B - 2, B - 1]
    took = {}

    def padded(a):
        return np.pad(a, ((0, 0), (0, 0), (pad, pad), (pad, pad)))

    def attempt(what, fn):
        """-> (result or None, kernel names, refusal text or None): OVER a limit a clean refusal (CnnAmdError) is an allowed outcome"""
        try:
            out, names = large.launch_log(capi, T, fn)
            return out, names, None
        except capi.CnnAmdError as e:
            assert side == "over", f"{row_id} {what}: refused UNDER its limit: {e}"
            return None, [], str(e)

    x = large.fill_uniform(T, T.empty((B, Ci, H, W), device="cuda"), g, -0.4, 0.6)
    xs = x[sel].cpu().numpy()
    y = None
    if run["fwd"]:
        y = T.full((B, Co, Ho, Wo), 7.0, device="cuda")
        _, names, refused = attempt("forward", lambda: conv.forward(x, w, b, y))
        took["fwd"] = refused and "REFUSED" or "+".join(names)
        if passes["fwd"]:
            _check_log(row_id, side, "forward", passes["fwd"], names, refused)
        if not refused:
            assert_close(y[sel].cpu().numpy(), O.conv2d_forward(padded(xs), wn, bn_, s), REL_TOL, f"{row_id} {side}: forward, oracle slice")
            # nothing left unwritten: no element still holds the pre-fill (an output of exactly 7.0 does not occur on these inputs)
            assert all(not bool((y[i0:i1] == 7.0).any()) for i0, i1 in large.sample_chunks(B, ny1)), f"{row_id} {side}: y has unwritten elements"
    if lean:
        del y
        y = None
        if not run["wgrad"]:
            del x
            x = None
        large.release(T)
    dy = None
    if run["dgrad"] or run["wgrad"]:
        dy = y if (y is not None and not lean) else T.empty((B, Co, Ho, Wo), device="cuda")  # (the forward output's storage, re-filled)
        y = None
        large.fill_uniform(T, dy, g, -1.0, 1.0)
    if run["dgrad"]:
        dys = dy[sel].cpu().numpy()
        dx = T.full((B, Ci, H, W), 7.0, device="cuda")
        _, names, refused = attempt("data gradient", lambda: conv.backward_data(dy, w, dx))
        took["dgrad"] = refused and "REFUSED" or "+".join(names)
        if passes["dgrad"]:
            _check_log(row_id, side, "data gradient", passes["dgrad"], names, refused)
        dx_ref = None
        if not refused:
            dx_ref = O.conv2d_backward(padded(xs), dys, wn, s, need=(False, False, True))[2][:, :, pad : pad + H, pad : pad + W]
            assert_close(dx[sel].cpu().numpy(), dx_ref, REL_TOL, f"{row_id} {side}: data gradient, oracle slice")
        if relu:
            relu_in = capi.relu_forward(x)
            dxm = T.full((B, Ci, H, W), 7.0, device="cuda")
            _, names, refused_m = attempt("data gradient + ReLU'", lambda: conv.backward_data_relu(dy, w, relu_in, dxm))
            took["dgrad+relu"] = refused_m and "REFUSED" or "+".join(names)
            if passes["dgrad"]:
                _check_log(row_id, side, "data gradient + ReLU'", passes["dgrad"], names, refused_m)
            assert bool(refused_m) == bool(refused), (refused, refused_m)
            if not refused_m:
                assert_close(dxm[sel].cpu().numpy(), np.where(xs <= 0, np.float32(0), dx_ref), REL_TOL, f"{row_id} {side}: data gradient + ReLU', oracle slice")
                # the samples the slice does not reach: the ReLU' form is the plain form masked (same sums, bit for bit), nothing unwritten
                zero = T.zeros((), device="cuda")
                assert large.equal_in_chunks(T, B, nx1, dxm, lambda i0, i1: T.where(relu_in[i0:i1] <= 0, zero, dx[i0:i1])), f"{row_id} {side}: dxm != masked dx"
            del relu_in, dxm
        elif not refused:
            # nothing left unwritten: no element still holds the pre-fill (a gradient of exactly 7.0 does not occur on these inputs)
            assert all(not bool((dx[i0:i1] == 7.0).any()) for i0, i1 in large.sample_chunks(B, nx1)), f"{row_id} {side}: dx has unwritten elements"
        del dx
        large.release(T)
    if run["wgrad"]:
        sel3 = [0, B // 2, B - 1]
        dys3 = dy[sel3].clone()
        keep = dy
        assert not lean
        dz = T.zeros((B, Co, Ho, Wo), device="cuda")
        dz[sel3] = dys3
        gw, gb = T.full((Co, Ci, k, k), 7.0, device="cuda"), T.full((Co,), 7.0, device="cuda")
        _, names, refused = attempt("weight gradient", lambda: conv.backward_weight(x, dz, float(B), gw, gb))
        took["wgrad"] = refused and "REFUSED" or "+".join(names)
        if passes["wgrad"]:
            _check_log(row_id, side, "weight gradient", passes["wgrad"], names, refused)
        del dz
        if not refused:
            gw_ref, gb_ref, _ = O.conv2d_backward(padded(x[sel3].cpu().numpy()), dys3.cpu().numpy(), np.zeros((Co, Ci, k, k), np.float32), s,
                                                  need=(True, True, False))
            assert_close(gw.cpu().numpy(), gw_ref * np.float32(3.0 / B), REL_TOL, f"{row_id} {side}: weight gradient, oracle slice")
            assert_close(gb.cpu().numpy(), gb_ref * np.float32(3.0 / B), REL_TOL, f"{row_id} {side}: bias gradient, oracle slice")
            # all samples live: the gradient is linear in dy (exact: every product and partial sum doubles)
            gw1, gb1 = conv.backward_weight(x, keep, float(B))
            gw1, gb1 = gw1.clone(), gb1.clone()
            keep.mul_(2.0)
            gw2, gb2 = conv.backward_weight(x, keep, float(B))
            assert T.equal(gw2, gw1 * 2.0) and T.equal(gb2, gb1 * 2.0), f"{row_id} {side}: weight gradient not exactly linear in dy"
    T.cuda.synchronize()
    peak = T.cuda.max_memory_allocated()
    large.report(row=row_id, side=side, B=B, footprint_gib=round(footprint / GIB, 2), peak_gib=round(peak / GIB, 2), seconds=round(time.time() - t0, 1),
                 **{"took_" + p: v for p, v in took.items()})
    del x, dy, conv
    large.release(T)


def _flat_chunks(n, step=1 << 27):
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def test_relu_beyond_2_31_elements(T):
    """tier B: ReLU forward / backward (relu.cpp:25, :37-39) on n = 2^31 + 5 elements -- the float4 body's index passes 2^29, the element
    index 2^31, and the scalar tail holds the last element: the whole tensor against clamp_min(0) / where(y <= 0, 0, dy) on the device, bit
    for bit; the last 2^16 + 5 elements against the oracle, bit for bit"""
    from cnn_amd import capi

    n = L31 + 5
    footprint = 4 * 4 * n + 4 * (1 << 27) * 4
    large.require_memory(T, footprint, "relu")
    t0 = time.time()
    g = T.Generator(device="cuda").manual_seed(31)
    x = large.fill_uniform(T, T.empty((n,), device="cuda"), g, -0.4, 0.6)
    y = T.full((n,), 7.0, device="cuda")
    _, names_f = large.launch_log(capi, T, lambda: capi.relu_forward(x, y))
    assert "relu_fwd_vec" in names_f and "relu_fwd_scalar" in names_f, names_f
    assert all(T.equal(y[a:b], x[a:b].clamp_min(0)) for a, b in _flat_chunks(n)), "relu forward"
    dy = large.fill_uniform(T, T.empty((n,), device="cuda"), g, -1.0, 1.0)
    dy0 = dy.clone()
    _, names_b = large.launch_log(capi, T, lambda: capi.relu_backward(y, dy))
    assert "relu_bwd_vec" in names_b and "relu_bwd_scalar" in names_b, names_b
    zero = T.zeros((), device="cuda")
    assert all(T.equal(dy[a:b], T.where(y[a:b] <= 0, zero, dy0[a:b])) for a, b in _flat_chunks(n)), "relu backward"
    tail = slice(n - (1 << 16) - 5, n)
    xt = x[tail].cpu().numpy()
    y_o = O.relu_forward(xt)
    assert np.array_equal(y[tail].cpu().numpy().view(np.uint32), y_o.view(np.uint32))
    assert np.array_equal(dy[tail].cpu().numpy().view(np.uint32), O.relu_backward(y_o, dy0[tail].cpu().numpy()).view(np.uint32))
    large.report(row="B-relu", side="over", n=n, footprint_gib=round(footprint / GIB, 2), peak_gib=round(T.cuda.max_memory_allocated() / GIB, 2),
                 seconds=round(time.time() - t0, 1), took_fwd="+".join(names_f), took_bwd="+".join(names_b))
    del x, y, dy, dy0
    large.release(T)


def test_maxpool_2x2_beyond_2_31_elements(T):
    """tier B: MaxPool2D(2, 2) forward / backward / backward + ReLU' (pool2d.cpp:60-83, :100-107, relu.cpp:37) with B*C*H*W > 2^31 (16
    channels of 112 x 112: C*H*W stays far below the int32 mask's range).  Whole tensor on the device against exact restatements: the
    pooled tensor is the window maximum; the mask names an element of ITS window of its channel that holds that maximum; the backward pass
    is the scatter of the deltas to the masked elements (zeros elsewhere: every element written).  The last two samples against the
    oracle bit for bit, mask -- i.e. the tie rule -- included."""
    from cnn_amd import capi

    C, H, W = 16, 112, 112
    B = batch_under(C * H * W, L31) + 1
    assert B == 10700 and B * C * H * W > L31
    n, npool = B * C * H * W, B * C * (H // 2) * (W // 2)
    footprint = 4 * (2 * n + 3 * npool) + 8 * (1 << 27) * 4
    large.require_memory(T, footprint, "maxpool")
    t0 = time.time()
    g = T.Generator(device="cuda").manual_seed(37)
    x = large.fill_uniform(T, T.empty((B, C, H, W), device="cuda"), g, -0.4, 0.6)
    (pooled, mask), names_f = large.launch_log(capi, T, lambda: capi.maxpool_forward(x, 2, 2))
    PH, PW = H // 2, W // 2
    # the window (c, ph, pw) in the mask's frame: index into the SAMPLE (pool2d.cpp:81)
    corner = (T.arange(C, device="cuda").view(C, 1, 1) * (H * W) + T.arange(PH, device="cuda").view(1, PH, 1) * (2 * W)
              + T.arange(PW, device="cuda").view(1, 1, PW) * 2)
    for i0, i1 in large.sample_chunks(B, C * H * W):
        xc = x[i0:i1]
        assert T.equal(pooled[i0:i1], xc.view(i1 - i0, C, PH, 2, PW, 2).amax((3, 5))), f"pooled tensor, samples {i0}..{i1}"
        m = mask[i0:i1].long()
        off = m - corner
        assert bool(((off == 0) | (off == 1) | (off == W) | (off == W + 1)).all()), f"mask outside its window, samples {i0}..{i1}"
        assert T.equal(xc.reshape(i1 - i0, -1).gather(1, m.view(i1 - i0, -1)).view_as(m), pooled[i0:i1]), f"mask does not name the maximum, samples {i0}..{i1}"
    dpool = large.fill_uniform(T, T.empty_like(pooled), g, -1.0, 1.0)
    dx = T.full((B, C, H, W), 7.0, device="cuda")
    _, names_b = large.launch_log(capi, T, lambda: capi.maxpool_backward(dpool, mask, (B, C, H, W), 2, 2, dx))
    zero = T.zeros((), device="cuda")

    def scatter_of(d, i0, i1):
        out = T.zeros((i1 - i0, C * H * W), device="cuda")
        out.scatter_(1, mask[i0:i1].long().view(i1 - i0, -1), d.reshape(i1 - i0, -1))
        return out.view(i1 - i0, C, H, W)

    assert large.equal_in_chunks(T, B, C * H * W, dx, lambda i0, i1: scatter_of(dpool[i0:i1], i0, i1)), "maxpool backward"
    dx.fill_(7.0)
    _, names_r = large.launch_log(capi, T, lambda: capi.maxpool_backward_relu(dpool, mask, pooled, (B, C, H, W), 2, 2, dx))
    assert large.equal_in_chunks(T, B, C * H * W, dx, lambda i0, i1: scatter_of(T.where(pooled[i0:i1] <= 0, zero, dpool[i0:i1]), i0, i1)), "maxpool backward + ReLU'"
    last = slice(B - 2, B)
    xl, dl = x[last].cpu().numpy(), dpool[last].cpu().numpy()
    p_o, m_o = O.maxpool_forward(xl, 2, 2)
    assert np.array_equal(pooled[last].cpu().numpy().view(np.uint32), p_o.view(np.uint32)) and np.array_equal(mask[last].cpu().numpy(), m_o)
    dr_o = O.maxpool_backward(np.where(p_o <= 0, np.float32(0), dl), m_o, (2, C, H, W), 2, 2)
    assert np.array_equal(dx[last].cpu().numpy().view(np.uint32), dr_o.view(np.uint32))
    large.report(row="B-maxpool", side="over", B=B, footprint_gib=round(footprint / GIB, 2), peak_gib=round(T.cuda.max_memory_allocated() / GIB, 2),
                 seconds=round(time.time() - t0, 1), took_fwd="+".join(names_f), took_bwd="+".join(names_b), took_bwd_relu="+".join(names_r))
    del x, pooled, mask, dpool, dx
    large.release(T)


def test_batchnorm_beyond_2_31_elements(T):
    """tier B: BatchNorm2D training forward / backward and the pooled forms with B*C*H*W > 2^31 and a small C*H*W (16 channels of 56 x 56,
    134 M elements per channel), after test_batchnorm_full_size_properties: batch statistics and moving statistics against float64 sums
    gathered on the device, y's per-channel mean / variance, the parameter gradients against float64 sums, dx against the float64 closed
    form of batchnorm2d.cpp:118-155 on the first and last samples; then BatchNorm -> ReLU -> MaxPool in one apply pass and the backward
    pass from the pooled domain, each bit-identical to the sequence it replaces, whole tensors on the device"""
    from cnn_amd import capi
    from tests.util import rel_err

    C, H, W = 16, 56, 56
    B = batch_under(C * H * W, L31) + 1
    assert B * C * H * W > L31
    n, npool = B * C * H * W, B * C * (H // 2) * (W // 2)
    footprint = 4 * (3 * n + 4 * npool) + 8 * GIB  # (x, y, relu(y) + two pooled tensors and masks at the peak; float64 chunk temporaries)
    large.require_memory(T, footprint, "batchnorm")
    t0 = time.time()
    g = T.Generator(device="cuda").manual_seed(41)
    x = large.fill_uniform(T, T.empty((B, C, H, W), device="cuda"), g, -2.0, 4.0)  # (mean 1, sigma 1.73: full_size_properties' scale)
    gamma = T.rand(C, device="cuda", generator=g) + 0.5
    beta = T.rand(C, device="cuda", generator=g) - 0.5
    mm, mv = T.zeros(C, device="cuda"), T.zeros(C, device="cuda")
    bn = capi.BatchNorm2d(B, C, H, W)
    assert bn.backward_pooled_supported() and capi.load().cnn_batchnorm2d_forward_relu_pool_supported(B, C, H, W)
    chunks = large.sample_chunks(B, C * H * W)
    L = B * H * W

    def chan_sum(f):
        """sum over (batch, plane) of f(i0, i1) -> [C] float64, accumulated in sample chunks"""
        acc = T.zeros(C, dtype=T.float64, device="cuda")
        for i0, i1 in chunks:
            acc += f(i0, i1).sum(dim=(0, 2, 3))
        return acc

    cv = lambda t: t.view(1, C, 1, 1)
    mean_ref = chan_sum(lambda a, b: x[a:b].double()) / L
    var_ref = chan_sum(lambda a, b: (x[a:b].double() - cv(mean_ref)) ** 2) / L
    y, r = T.full_like(x, 7.0), T.full_like(x, 7.0)
    _, names_f = large.launch_log(capi, T, lambda: bn.forward(x, gamma, beta, mm, mv, y, training=True, y_relu=r))
    host = lambda t: t.detach().cpu().numpy()
    assert_close(host(bn.saved_mean), host(mean_ref), REL_TOL, "B-batchnorm: batch mean vs float64")
    assert_close(host(bn.saved_var), host(var_ref), REL_TOL, "B-batchnorm: batch variance vs float64")
    assert_close(host(mm), 0.1 * host(mean_ref), REL_TOL, "B-batchnorm: moving mean vs float64")
    assert_close(host(mv), 0.1 * host(var_ref), REL_TOL, "B-batchnorm: moving variance vs float64")
    y_mean = chan_sum(lambda a, b: y[a:b].double()) / L
    y_var = chan_sum(lambda a, b: (y[a:b].double() - cv(y_mean)) ** 2) / L
    assert (y_mean - beta.double()).abs().max().item() < 1e-4
    assert_close(host(y_var), host(gamma.double() ** 2 * var_ref / (var_ref + 1e-5)), REL_TOL, "B-batchnorm: variance of y")
    assert all(T.equal(r[a:b], y[a:b].clamp_min(0)) for a, b in chunks), "y_relu != relu(y)"
    # the oracle's own arithmetic on the elements of the last sample, with the statistics of the whole batch: y = gamma * norm + beta
    sd_ref = T.sqrt(var_ref + 1e-5)
    norm_of = lambda a, b: (x[a:b].double() - cv(mean_ref)) / cv(sd_ref)
    for a, b in ((0, 1), (B - 1, B)):
        assert_close(host(y[a:b]), host(norm_of(a, b) * cv(gamma.double()) + cv(beta.double())), REL_TOL, f"B-batchnorm: y of sample {a} vs float64")
    # pooled forward: one apply pass, bit-identical to forward_relu + maxpool_forward
    pooled, mask = capi.maxpool_forward(r, 2, 2)
    bn2 = capi.BatchNorm2d(B, C, H, W)
    mm2, mv2 = T.zeros(C, device="cuda"), T.zeros(C, device="cuda")
    p2, m2 = T.full_like(pooled, 7.0), T.full_like(mask, -3)
    _, names_fp = large.launch_log(capi, T, lambda: bn2.forward_relu_pool(x, gamma, beta, mm2, mv2, p2, m2, training=True))
    assert T.equal(p2, pooled) and T.equal(m2, mask) and T.equal(mm2, mm) and T.equal(mv2, mv)
    assert T.equal(bn2.saved_mean, bn.saved_mean) and T.equal(bn2.saved_var, bn.saved_var)
    del p2, m2, y
    # backward, from the pooled domain and as the sequence it replaces
    dpool = large.fill_uniform(T, T.empty_like(pooled), g, -1.0, 1.0)
    gg, gb, dx = T.full((C,), 7.0, device="cuda"), T.full((C,), 7.0, device="cuda"), T.full_like(x, 7.0)
    _, names_bp = large.launch_log(capi, T, lambda: bn.backward_pooled(x, dpool, mask, pooled, gamma, gg, gb, dx))
    assert names_bp == ["bn_bwd_stats+pool", "bn_bwd_apply+pool"], names_bp
    dy = capi.maxpool_backward_relu(dpool, mask, pooled, (B, C, H, W), 2, 2, r)  # (into the ReLU output's storage)
    del r
    gb_ref = chan_sum(lambda a, b: dy[a:b].double())
    gg_ref = chan_sum(lambda a, b: dy[a:b].double() * norm_of(a, b))
    dn_sum = gb_ref * gamma.double()
    dnn_sum = gg_ref * gamma.double()
    dx_of = lambda a, b: (dy[a:b].double() * cv(gamma.double()) - cv(dn_sum) / L - norm_of(a, b) * cv(dnn_sum) / L) / cv(sd_ref)
    dx_refs = [host(dx_of(a, b)) for a, b in ((0, 1), (B - 1, B))]
    gg3, gb3 = T.full((C,), 7.0, device="cuda"), T.full((C,), 7.0, device="cuda")
    _, names_b = large.launch_log(capi, T, lambda: bn.backward(x, dy, gamma, gg3, gb3))  # (dy -> dx in place)
    assert_close(host(gb3), host(gb_ref), REL_TOL, "B-batchnorm: beta gradient vs float64")
    assert_close(host(gg3), host(gg_ref), REL_TOL, "B-batchnorm: gamma gradient vs float64")
    for (a, b), ref in zip(((0, 1), (B - 1, B)), dx_refs):
        assert_close(host(dy[a:b]), ref, REL_TOL, f"B-batchnorm: dx of sample {a} vs float64")
    assert T.equal(gg, gg3) and T.equal(gb, gb3), "pooled-domain parameter gradients differ from the sequence's"
    assert all(T.equal(dx[a:b], dy[a:b]) for a, b in chunks), "pooled-domain dx differs from the sequence's"
    large.report(row="B-batchnorm", side="over", B=B, footprint_gib=round(footprint / GIB, 2), peak_gib=round(T.cuda.max_memory_allocated() / GIB, 2),
                 seconds=round(time.time() - t0, 1), took_fwd="+".join(names_f), took_fwd_pool="+".join(names_fp), took_bwd="+".join(names_b),
                 took_bwd_pool="+".join(names_bp), rel_err_mean=rel_err(host(bn.saved_mean), host(mean_ref)))
    del x, dx, dy, pooled, mask, dpool
    large.release(T)


FIRST_BLOCK_LIMIT = ((1 << 31) - 16) // 4  # elements of a float tensor whose BYTE offsets stay below 2^31 - 16 (conv_direct.hip)


@pytest.mark.parametrize("side", ["under", "over"])
@pytest.mark.parametrize("tensor", ["y", "x"])
def test_first_block_on_both_sides_of_its_limits(T, tensor, side):
    """tier A, the first block 3 -> 16 @ 224, 3x3 / stride 2 (conv_direct.hip): its packed kernels address x and y = conv(x) through 32-bit
    byte offsets below 2^31 - 16.  The y limit binds first (B = 2723 / 2724: packed data gradient, its pooled-domain form and the packed
    one-byte pool mask), the x limit second (3566 / 3567: packed forward and with it the pool-fused forward).  Which form must run follows
    from the two documented limits alone.  Under a limit: the entry points of test_conv_relu_maxpool_fusion_is_bit_identical /
    test_packed_pool_mask_block_is_bit_identical hold their bit-identities over the WHOLE tensors (on the device).  Over it: the library
    takes the unfused / int32-mask / unpacked form or refuses (CnnAmdError) -- and what it computes still matches the oracle slices."""
    from cnn_amd import capi

    H = W = 224
    Ho = Wo = 111
    PH = PW = 55
    per = {"y": 16 * Ho * Wo, "x": 3 * H * W}[tensor]
    under = batch_under(per, FIRST_BLOCK_LIMIT)
    assert (under, under + 1) == {"y": (2723, 2724), "x": (3566, 3567)}[tensor]
    B = under if side == "under" else under + 1
    x_ok, y_ok = B * 3 * H * W < FIRST_BLOCK_LIMIT, B * 16 * Ho * Wo < FIRST_BLOCK_LIMIT
    assert {"y": y_ok, "x": x_ok}[tensor] == (side == "under") and B * 16 * PH * PW < FIRST_BLOCK_LIMIT
    nx, ny, npool = B * 3 * H * W, B * 16 * Ho * Wo, B * 16 * PH * PW
    footprint = 4 * (3 * nx + 3 * ny + 8 * npool) + 2 * GIB
    large.require_memory(T, footprint, f"first block {tensor} {side}")
    t0 = time.time()
    g = T.Generator(device="cuda").manual_seed(43)
    case = (B, 3, H, W, 16, 3, 2, 0)
    conv, packed = capi.Conv2d(*case), capi.Conv2d(*case)
    packed.set_pool_mask_packed()
    x = large.fill_uniform(T, T.empty((B, 3, H, W), device="cuda"), g, -0.4, 0.6)
    w = T.randn((16, 3, 3, 3), generator=g, device="cuda") * float(np.sqrt(2.0 / 27))
    b = T.randn((16,), generator=g, device="cuda") * 0.1
    wn, bn_ = w.cpu().numpy(), b.cpu().numpy()
    sel = [0, 1, B // 2, B - 2, B - 1]
    xs = x[sel].cpu().numpy()
    took = {}

    def refused(fn):
        try:
            fn()
        except capi.CnnAmdError:
            return True
        return False

    # forward + ReLU, and the pool behind it: the sequence the fused forms are held to
    y, r = T.full((B, 16, Ho, Wo), 7.0, device="cuda"), T.full((B, 16, Ho, Wo), 7.0, device="cuda")
    _, names = large.launch_log(capi, T, lambda: conv.forward_relu(x, w, b, y, r))
    took["fwd_relu"] = "+".join(names)
    assert ("conv_fwd_pk<3,16,3,2>+relu" in names) == x_ok and ("conv_direct_fwd<3,16,3,2>+relu" in names) == (not x_ok), (names, x_ok)
    assert_close(y[sel].cpu().numpy(), O.conv2d_forward(xs, wn, bn_, 2), REL_TOL, f"first block {tensor} {side}: forward, oracle slice")
    assert all(T.equal(r[a:c], y[a:c].clamp_min(0)) for a, c in large.sample_chunks(B, 16 * Ho * Wo)), "relu output"
    pooled_ref, mask_ref = capi.maxpool_forward(r, 2, 2)
    del y
    # pool-fused forward: needs the packed forward kernel (x limit)
    pooled, mask = T.full_like(pooled_ref, 7.0), T.full_like(mask_ref, -1)
    if x_ok:
        _, names = large.launch_log(capi, T, lambda: conv.relu_maxpool2_forward(x, w, b, pooled, mask))
        took["fwd_pool"] = "+".join(names)
        assert "conv_fwd_pool_pk<3,16,3,2>" in names, names
        assert T.equal(pooled, pooled_ref) and T.equal(mask & 0x7FFFFFFF, mask_ref) and T.equal(mask < 0, pooled_ref <= 0)
    else:
        assert not conv.relu_maxpool2_supported() and refused(lambda: conv.relu_maxpool2_forward(x, w, b, pooled, mask))
        took["fwd_pool"] = "REFUSED"
        pooled, mask = pooled_ref, T.where(pooled_ref <= 0, mask_ref | -0x80000000, mask_ref)  # (the marked form, built by hand)
    # packed one-byte mask: needs the packed forward AND the packed data gradient (both limits)
    mask8 = T.full((max(packed.pool_mask_bytes(), 64),), 0x55, dtype=T.uint8, device="cuda")
    pooled8 = T.full_like(pooled_ref, 7.0)
    if x_ok and y_ok:
        assert packed.pool_mask_packed_supported()
        _, names = large.launch_log(capi, T, lambda: packed.relu_maxpool2_forward(x, w, b, pooled8, mask8))
        took["fwd_pool_m8"] = "+".join(names)
        assert "conv_fwd_pool_pk<3,16,3,2>+m8" in names, names
        unpacked = T.full_like(mask, -2)
        packed.pool_mask_unpack(mask8, unpacked)
        assert T.equal(pooled8, pooled_ref) and T.equal(unpacked, mask)
        del unpacked
    else:
        assert not packed.pool_mask_packed_supported() and refused(lambda: packed.relu_maxpool2_forward(x, w, b, pooled8, mask8))
        took["fwd_pool_m8"] = "REFUSED"
    del pooled8
    # data gradient: plain from the materialised delta (packed kernel under the y limit, row kernel over it), then from the pooled domain
    dpool = large.fill_uniform(T, T.empty_like(pooled_ref), g, -1.0, 1.0)
    dy = capi.maxpool_backward_relu(dpool, mask_ref, pooled_ref, (B, 16, Ho, Wo), 2, 2, r)  # (into the ReLU output's storage)
    del r
    dx_ref = T.full((B, 3, H, W), 7.0, device="cuda")
    _, names = large.launch_log(capi, T, lambda: conv.backward_data(dy, w, dx_ref))
    took["dgrad"] = "+".join(names)
    assert ("conv_dgrad_pk<3,16,3,2>" in names) == y_ok and ("conv_direct_dgrad<3,16,3,2>" in names) == (not y_ok), (names, y_ok)
    dx_o = O.conv2d_backward(xs, dy[sel].cpu().numpy(), wn, 2, need=(False, False, True))[2]
    assert_close(dx_ref[sel].cpu().numpy(), dx_o, REL_TOL, f"first block {tensor} {side}: data gradient, oracle slice")
    dx = T.full((B, 3, H, W), 7.0, device="cuda")
    if x_ok and y_ok:
        _, names = large.launch_log(capi, T, lambda: conv.backward_data_pooled2(dpool, mask, None, w, dx))
        took["dgrad_pool"] = "+".join(names)
        assert "conv_dgrad_pk<3,16,3,2>+poolm" in names, names
        assert T.equal(dx, dx_ref), "pooled-domain data gradient differs from the sequence's"
        dx.fill_(7.0)
        _, names = large.launch_log(capi, T, lambda: packed.backward_data_pooled2(dpool, mask8, None, w, dx))
        took["dgrad_pool_m8"] = "+".join(names)
        assert "conv_dgrad_pk<3,16,3,2>+poolm8" in names, names
        assert T.equal(dx, dx_ref), "packed-mask data gradient differs from the sequence's"
    else:
        assert refused(lambda: conv.backward_data_pooled2(dpool, mask, None, w, dx)), "pooled-domain data gradient over a limit of its kernels"
        took["dgrad_pool"] = "REFUSED"
    del dx, dx_ref
    # weight gradient: a delta that is zero except on three samples against the oracle; from the pooled domain bit-identical to it
    sel3 = [0, B // 2, B - 1]
    dpool3 = T.zeros_like(dpool)
    dpool3[sel3] = dpool[sel3]
    dy3 = capi.maxpool_backward_relu(dpool3, mask_ref, pooled_ref, (B, 16, Ho, Wo), 2, 2, dy)
    gw_ref, gb_ref = T.full((16, 3, 3, 3), 7.0, device="cuda"), T.full((16,), 7.0, device="cuda")
    _, names = large.launch_log(capi, T, lambda: conv.backward_weight(x, dy3, float(B), gw_ref, gb_ref))
    took["wgrad"] = "+".join(names)
    gw_o, gb_o, _ = O.conv2d_backward(x[sel3].cpu().numpy(), dy3[sel3].cpu().numpy(), np.zeros((16, 3, 3, 3), np.float32), 2, need=(True, True, False))
    assert_close(gw_ref.cpu().numpy(), gw_o * np.float32(3.0 / B), REL_TOL, f"first block {tensor} {side}: weight gradient, oracle slice")
    assert_close(gb_ref.cpu().numpy(), gb_o * np.float32(3.0 / B), REL_TOL, f"first block {tensor} {side}: bias gradient, oracle slice")
    gw, gb = T.full_like(gw_ref, 7.0), T.full_like(gb_ref, 7.0)
    if x_ok:
        _, names = large.launch_log(capi, T, lambda: conv.backward_weight_pooled2(x, dpool3, mask, None, float(B), gw, gb))
        took["wgrad_pool"] = "+".join(names)
        assert T.equal(gw, gw_ref) and T.equal(gb, gb_ref), "pooled-domain weight gradient differs from the sequence's"
    else:
        assert refused(lambda: conv.backward_weight_pooled2(x, dpool3, mask, None, float(B), gw, gb))
        took["wgrad_pool"] = "REFUSED"
    large.report(row="A-first-block-" + tensor, side=side, B=B, footprint_gib=round(footprint / GIB, 2), peak_gib=round(T.cuda.max_memory_allocated() / GIB, 2),
                 seconds=round(time.time() - t0, 1), **{"took_" + k: v for k, v in took.items()})
    del x, dy, dy3, dpool, dpool3, pooled, mask, pooled_ref, mask_ref, mask8
    large.release(T)


@pytest.mark.parametrize("case,words", [((8388608, 4, 64, 3, 8, 3, 1, 0), "row index"), ((715826518, 1, 1, 3, 1, 3, 1, 1), "too many output pixels")],
                         ids=["B*C*H=2^31", "B*Ho*Wo=2^31-4094"])
def test_implicit_gemm_refuses_what_its_int32_indices_cannot_hold(T, case, words):
    """tier B: the implicit GEMM indexes input rows (B*C*H) and output pixels (B*Ho*Wo) in int32 and must REFUSE beyond them
    (conv_igemm.hip make_plan), on 3-column planes that no other family takes.  The call is made on real full-size tensors: a missing
    guard would show as a wrong answer or a success, never as an access outside an allocation."""
    import ctypes

    from cnn_amd import capi

    B, Ci, H, W, Co, k, s, pad = case
    Ho, Wo = capi.conv_out_dim(H, k, s, pad), capi.conv_out_dim(W, k, s, pad)
    assert B * Ci * H >= L31 or B * Ho * Wo >= L31 - 4096
    nx, ny = B * Ci * H * W, B * Co * Ho * Wo
    ws_bytes = 256 << 20
    footprint = 4 * (nx + ny) + ws_bytes
    large.require_memory(T, footprint, "implicit GEMM refusal")
    x = T.zeros((B, Ci, H, W), device="cuda")
    y = T.full((B, Co, Ho, Wo), 7.0, device="cuda")
    w, b = T.ones((Co, Ci, k, k), device="cuda"), T.zeros((Co,), device="cuda")
    ws = T.empty(ws_bytes, dtype=T.uint8, device="cuda")
    desc = capi.ConvDesc(B, Ci, H, W, Co, k, s, pad)
    L = capi.load()
    with pytest.raises(capi.CnnAmdError, match=words):
        capi.check(L.cnn_conv2d_forward(ctypes.byref(desc), capi._ptr(x), capi._ptr(w), capi._ptr(b), capi._ptr(y), capi._ptr(ws), ws_bytes,
                                        capi._stream()), "cnn_conv2d_forward")
    T.cuda.synchronize()
    assert bool((y[-1] == 7.0).all()) and bool((y[0] == 7.0).all())  # (refused before anything ran)
    large.report(row="B-igemm-refusal", side="over", case=case, footprint_gib=round(footprint / GIB, 2), peak_gib=round(T.cuda.max_memory_allocated() / GIB, 2))
    del x, y, ws
    large.release(T)
