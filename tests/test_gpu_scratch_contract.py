"""Every caller-provided scratch buffer of the C ABI held to its size contract (tests/guarded.py).

The parity tests check input -> output.  Here every workspace, prepared-filter image and pool mask is EXACTLY as large as its
*_bytes query says, lies between two canary zones and is poisoned before every call, once with quiet NaNs and once with the bytes
0x5A (the float 1.5e16).  Two kinds of error show that a plain torch.empty() hides:
  * a store past the promised size (a canary byte changes: the failure names the desc, the call and the offset of the first byte);
  * a read of scratch this call never wrote -- a slab, a split-K partial tensor, a stage-1 row of the slab reduction -- which carries
    the poison into a result and misses the oracle.
Reference: the CPU oracle as in tests/test_gpu_parity.py (_oracle_conv), tests.util.assert_close at REL_TOL; the fused forms against
the composition their bit-identity tests use, under the same poison.  Calls whose digests tests/golden/conv_routes.json pins (they are
known to repeat) must give the same bits under both poisons.

Short buffers (told_bytes < the query's answer, same allocation, same poison): a call either refuses with a status or falls through
to a route that lives with less and returns the oracle's result; either way no byte beyond told_bytes changes.

Descs: tests/conv_route_cases.HAND_PICKED (the smallest plane per kernel family and boundary), its three OPTIONS over OPTION_CASES, and
two more that HAND_PICKED does not reach (each asserts from its own launch log that it got there):
  * (5, 64, 28, 28, 128, 3, 1, 1): wgrad_sp<28> writes 70 slabs of 128 x 577 floats -- more than 64 slabs of more than 65536 floats, the
    smallest batch of that plane at which reduce_slabs takes its two-stage form (slab_reduce/stage1 into the rows behind the slabs);
  * (2, 128, 30, 30, 512, 3, 1, 1) with IGEMM_CFG=232: no rule-based plan splits K, the tuner pins such tiles; 5 pixel tiles x 4 channel
    blocks x 8 channel ranges is the smallest forward this tile accepts (20 workgroups < CUs, 160 within a round, 16 chunks >= 2 x 8):
    8 partial tensors behind the filter image, in the workspace and in the prepared buffer (split_reduce/fwd);
  * (1, 12, 30, 30, 40, 3, 1, 1) with IGEMM_CFG=202, 226 and 22: three tiles only the tuner pins (tests/test_gpu_igemm_tiles.py holds all
    of them to exact bits): ragged 16-byte row units, whole-image staging with masked taps, the single-buffered kernel.

A HIP error (a status >= CNN_AMD_E_HIP, or a failed synchronisation) is not a refusal: the test then ends the whole session with
pytest.exit(returncode=3), because nothing more is to be started on a device that has faulted -- the tests behind it do not run."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import conv_route_cases as R
from tests import guarded
from tests.adam_ref import ref_clip, ref_total_norm
from tests.test_gpu_batchnorm import BN_SHAPES, POOLED_SHAPES
from tests.util import REL_TOL, assert_close, normal_scaled, uniform01, uniform_pm1

pytestmark = pytest.mark.gpu

STAGE1_CASE = (5, 64, 28, 28, 128, 3, 1, 1)
SPLITK_CASE = (2, 128, 30, 30, 512, 3, 1, 1)
SPLITK_OPTIONS = (("IGEMM_CFG", "232"), ("DGRAD_RD", "0"), ("CONV_ROWS", "0"))
# three tiles the tuner can pin and no rule picks on this plane (tests/igemm_tiles.py), forced on a 900-pixel plane with a 4-channel last
# chunk: 202 stages padded rows in 16-byte units with a ragged tail, 226 whole images with masked taps, 22 is single-buffered
TILE_CASE = (1, 12, 30, 30, 40, 3, 1, 1)
TILE_OPTIONS = {cfg: (("IGEMM_CFG", str(cfg)), ("CONV_ROWS", "0"), ("FWD_RD", "0"), ("DGRAD_RD", "0")) for cfg in (202, 226, 22)}
TILE_KERNELS = {202: "igemm_dma_kernel<32,2,2,1,4,4>", 226: "igemm_dma_kernel<32,2,1,1,4,4,img+mask>", 22: "igemm_kernel<32,2,1,2,2,16>"}
# (appended at the end: the seeds of the entries in front are derived from their index)
PARAMS = ([(c, ()) for c in R.HAND_PICKED] + [(STAGE1_CASE, ()), (SPLITK_CASE, SPLITK_OPTIONS)] +
          [(c, (opt,)) for opt in R.OPTIONS for c in R.OPTION_CASES] + [(TILE_CASE, TILE_OPTIONS[cfg]) for cfg in (202, 226, 22)])
# kernels the added descs exist for: {call: a name its launch log must hold}
MUST_LAUNCH = {(STAGE1_CASE, ()): {"backward_weight": "slab_reduce/stage1", "backward": "slab_reduce/stage1", "backward_prepared": "slab_reduce/stage1"},
               (SPLITK_CASE, SPLITK_OPTIONS): {"forward": "split_reduce/fwd", "forward_relu": "split_reduce/fwd+relu",
                                               "forward_prepared": "split_reduce/fwd+relu"}}
for _cfg, _kernel in TILE_KERNELS.items():
    MUST_LAUNCH[(TILE_CASE, TILE_OPTIONS[_cfg])] = {
        "forward": _kernel + "/fwd", "forward_relu": _kernel + "/fwd+relu", "forward_prepared": _kernel + "/fwd+relu",
        "backward_data": _kernel + "/dgrad", "backward_data_relu": _kernel + "/dgrad+relu",
        "backward_data_prepared": _kernel + "/dgrad", "backward_data_relu_prepared": _kernel + "/dgrad+relu"}


def _id(p):
    case, opts = p
    return R.key(case).replace(",", "_") + "".join(f"-{n}={v}" for n, v in opts)


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    assert capi.load().cnn_amd_device_arch().decode() == "gfx950"
    return torch


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")) as f:
        return json.load(f)


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Refused(Exception):
    pass


class Run:
    """one desc under one poison: the Conv2d object with every buffer replaced by a guarded one of the exact size"""

    def __init__(self, T, case, poison, data, problems, place=None):
        """place: how the operands reach the device -- None: plain uploads (dev); tests/test_gpu_operand_contract.py passes an object with
        .label, .guards and place(name, array) -> tensor that puts every operand between poison, and its canaries are asked with the rest"""
        from cnn_amd import capi

        self.T, self.case, self.poison, self.problems = T, case, poison, problems
        self.place, self.where = place, poison if place is None else place.label
        self.operand_guards = [] if place is None else place.guards
        B, Ci, H, W, Co, k, s, pad = case[:8]
        self.conv = conv = capi.Conv2d(B, Ci, H, W, Co, k, s, pad)
        conv.desc.flags = case[8] if len(case) > 8 else 0
        self.lib, self.d = conv.lib, C.byref(conv.desc)
        q = lambda f: int(getattr(self.lib, f)(self.d))
        self.sizes = {"ws": q("cnn_conv2d_workspace_bytes"), "bwd": q("cnn_conv2d_backward_workspace_bytes"),
                      "im2col": q("cnn_conv2d_im2col_workspace_bytes"), "prepared": q("cnn_conv2d_prepared_bytes")}
        assert all(v > 0 for v in self.sizes.values()), self.sizes
        self.ws = guarded.scratch(self.sizes["ws"], poison=poison, name="ws")
        self.bwd = guarded.scratch(self.sizes["bwd"], poison=poison, name="backward ws")
        self.im2col = guarded.scratch(self.sizes["im2col"], poison=poison, name="im2col ws")
        self.pf = guarded.scratch(self.sizes["prepared"], poison=poison, name="prepared fwd")
        self.pd = guarded.scratch(self.sizes["prepared"], poison=poison, name="prepared dgrad")
        conv.ws, conv.ws_bytes = self.ws.view, self.sizes["ws"]
        conv._bwd_ws, conv._im2col_ws = self.bwd.view, self.im2col.view
        self.scratch = [self.ws, self.bwd, self.im2col, self.pf, self.pd]
        self.repoison = [self.ws, self.bwd, self.im2col]  # (the prepared images: before prepare_filters only)
        self.x, self.w, self.b, self.dy, self.relu_below = (self.operand(n, a) for n, a in zip(("x", "w", "b", "dy", "relu_below"), data))
        self.out_shape, self.x_shape, self.w_shape = conv.out_shape(), (B, Ci, H, W), (Co, Ci, k, k)
        self.results, self.logs = {}, {}

    def operand(self, name, array):
        return dev(self.T, array) if self.place is None else self.place(name, array)

    def out(self, shape, keep, dtype=None):
        return guarded.output(shape, self.poison, keep, dtype=dtype)

    def call(self, name, fn, extra=(), refill=()):
        """re-poison, call, synchronise, ask every guard; -> {output name: numpy} | None when the library refused"""
        from cnn_amd import capi

        for g in self.repoison + list(refill):
            g.refill()
        keep = []
        try:
            outs = fn(keep)
        except capi.CnnAmdError as e:
            _stop_on_device_error(e)
            outs = None
            self.results[name] = Refused(str(e))
        try:
            self.T.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error behind {name} of desc {self.case}: {e}", returncode=3)
        for msg in guarded.check(self.scratch + self.operand_guards + keep + list(extra)):
            self.problems.append(f"{name} [{self.where}]: {msg}")
        self.logs[name] = {key.split("|")[0] for key in capi.kernel_timing_report()}  # (the launch log is on for the whole case)
        if outs is not None:
            self.results[name] = {k: host(v) for k, v in outs.items()}
        return self.results[name] if outs is not None else None


def _stop_on_device_error(e):
    """a refusal is a status below CNN_AMD_E_HIP; a HIP error ends the session: nothing more is started on a device that has faulted"""
    import re

    m = re.search(r"failed with code (-?\d+)", str(e))
    if m and int(m.group(1)) >= 1000:
        pytest.exit(f"HIP error: {e}", returncode=3)


def _close(problems, tag, got, ref):
    try:
        assert_close(got, ref, REL_TOL, tag)
    except AssertionError as e:
        problems.append(str(e))


def _same(problems, tag, a, b):
    if a.shape != b.shape or not np.array_equal(bits(a), bits(b)):
        problems.append(f"{tag}: not bit-identical")


def _plain_calls(r):
    """the unprepared calls, the combined backward, im2col"""
    from cnn_amd import capi

    conv, lib, d = r.conv, r.lib, r.d
    div = float(r.case[0])
    P, S = capi._ptr, capi._stream

    def forward_relu(keep):
        y, yr = r.out(r.out_shape, keep), r.out(r.out_shape, keep)
        conv.forward_relu(r.x, r.w, r.b, y, yr)
        return {"y": y, "y_relu": yr}

    def backward_weight(keep):
        gw, gb = conv.backward_weight(r.x, r.dy, div, gw=r.out(r.w_shape, keep), gb=r.out(r.w_shape[:1], keep))
        return {"gw": gw, "gb": gb}

    def backward(defer):
        def fn(keep):
            gw, gb, dx = conv.backward(r.x, r.dy, r.w, div, gw=r.out(r.w_shape, keep), gb=r.out(r.w_shape[:1], keep), dx=r.out(r.x_shape, keep),
                                       defer_join=defer)
            if defer:
                capi.side_stream_join()
            return {"gw": gw, "gb": gb, "dx": dx}
        return fn

    def forward_im2col(keep):
        y = r.out(r.out_shape, keep)
        capi.check(lib.cnn_conv2d_forward_im2col(d, P(r.x), P(r.w), P(r.b), P(y), P(r.im2col.view), r.sizes["im2col"], S()), "cnn_conv2d_forward_im2col")
        return {"y": y}

    def backward_weight_im2col(keep):
        gw, gb = r.out(r.w_shape, keep), r.out(r.w_shape[:1], keep)
        capi.check(lib.cnn_conv2d_backward_weight_im2col(d, P(r.x), P(r.dy), P(gw), P(gb), div, P(r.im2col.view), r.sizes["im2col"], S()),
                   "cnn_conv2d_backward_weight_im2col")
        return {"gw": gw, "gb": gb}

    def backward_data_im2col(keep):
        dx = r.out(r.x_shape, keep)
        capi.check(lib.cnn_conv2d_backward_data_im2col(d, P(r.dy), P(r.w), P(dx), P(r.im2col.view), r.sizes["im2col"], S()),
                   "cnn_conv2d_backward_data_im2col")
        return {"dx": dx}

    return {
        "forward": lambda keep: {"y": conv.forward(r.x, r.w, r.b, r.out(r.out_shape, keep))},
        "forward_relu": forward_relu,
        "backward_data": lambda keep: {"dx": conv.backward_data(r.dy, r.w, r.out(r.x_shape, keep))},
        "backward_data_relu": lambda keep: {"dx": conv.backward_data_relu(r.dy, r.w, r.relu_below, r.out(r.x_shape, keep))},
        "backward_weight": backward_weight,
        "backward": backward(False),
        "backward/defer_join": backward(True),
        "forward_im2col": forward_im2col,
        "backward_weight_im2col": backward_weight_im2col,
        "backward_data_im2col": backward_data_im2col,
    }


def _prepared_calls(r):
    from cnn_amd import capi

    conv, lib, d = r.conv, r.lib, r.d
    div = float(r.case[0])
    P, S = capi._ptr, capi._stream
    pf, pd = r.pf.view, r.pd.view

    def forward_prepared(keep):
        y, yr = r.out(r.out_shape, keep), r.out(r.out_shape, keep)
        conv.forward_prepared(r.x, pf, r.b, y, yr)
        return {"y": y, "y_relu": yr}

    def backward_prepared(relu):
        def fn(keep):
            gw, gb, dx = r.out(r.w_shape, keep), r.out(r.w_shape[:1], keep), r.out(r.x_shape, keep)
            if relu:
                capi.check(lib.cnn_conv2d_backward_prepared_relu(d, P(r.x), P(r.dy), P(pd), P(r.relu_below), P(gw), P(gb), P(dx), div, P(r.ws.view),
                                                                 r.sizes["ws"], S(), 0), "cnn_conv2d_backward_prepared_relu")
            else:
                capi.check(lib.cnn_conv2d_backward_prepared(d, P(r.x), P(r.dy), P(pd), P(gw), P(gb), P(dx), div, P(r.ws.view), r.sizes["ws"], S(), 0),
                           "cnn_conv2d_backward_prepared")
            return {"gw": gw, "gb": gb, "dx": dx}
        return fn

    return {
        "forward_prepared": forward_prepared,
        "backward_data_prepared": lambda keep: {"dx": conv.backward_data_prepared(r.dy, pd, r.out(r.x_shape, keep))},
        "backward_data_relu_prepared": lambda keep: {"dx": conv.backward_data_relu(r.dy, None, r.relu_below, r.out(r.x_shape, keep), prepared_dgrad=pd)},
        "backward_prepared": backward_prepared(False),
        "backward_prepared_relu": backward_prepared(True),
    }


def _check_conv_results(r, ref, may_refuse):
    """every result of one Run against the oracle and the compositions"""
    y_ref, gw_ref, gb_ref, dx_ref, dxm_ref = ref
    res, pr = r.results, r.problems
    tag = lambda call, what: f"{call} [{r.where}] {what}"
    expect = {"y": y_ref, "y_relu": np.maximum(y_ref, np.float32(0)), "gw": gw_ref, "gb": gb_ref}
    for call, outs in res.items():
        if isinstance(outs, Refused):
            if not may_refuse(call):
                pr.append(f"{call} [{r.where}]: refused with a full-size buffer: {outs}")
            continue
        if call.startswith("pool/"):
            continue
        for what, got in outs.items():
            want = (dxm_ref if "relu" in call else dx_ref) if what == "dx" else expect[what]
            _close(pr, tag(call, what), got, want)
        if "y_relu" in outs and not np.array_equal(outs["y_relu"], np.where(outs["y"] >= 0, outs["y"], np.float32(0))):  # (relu.cpp:25 on the call's own y)
            pr.append(tag(call, "y_relu != relu(y)"))
    # the combined backward == the separate calls, bit for bit (test_conv2d_combined_backward_matches_separate_calls), under poison
    sep_w, sep_d = res.get("backward_weight"), res.get("backward_data")
    for call in ("backward", "backward/defer_join", "backward_prepared"):
        both = res.get(call)
        if isinstance(both, dict) and isinstance(sep_w, dict) and isinstance(sep_d, dict):
            for what, sep in (("gw", sep_w["gw"]), ("gb", sep_w["gb"]), ("dx", sep_d["dx"])):
                _same(pr, tag(call, f"{what} == the separate call's"), both[what], sep)
    both, sep_m = res.get("backward_prepared_relu"), res.get("backward_data_relu")
    if isinstance(both, dict) and isinstance(sep_w, dict) and isinstance(sep_m, dict):
        for what, sep in (("gw", sep_w["gw"]), ("gb", sep_w["gb"]), ("dx", sep_m["dx"])):
            _same(pr, tag("backward_prepared_relu", f"{what} == the separate call's"), both[what], sep)


def _pool_family(r, packed):
    """the pool-fused first block with the int32 or the packed mask (a Conv2d of its own for the flag), every buffer guarded"""
    from cnn_amd import capi

    T, pr = r.T, r.problems
    B, Ci, H, W, Co, k, s, pad = r.case[:8]
    conv = capi.Conv2d(B, Ci, H, W, Co, k, s, pad)
    conv.set_pool_mask_packed(packed)
    q = lambda f: int(getattr(conv.lib, f)(C.byref(conv.desc)))
    n_ws, n_prep = q("cnn_conv2d_workspace_bytes"), q("cnn_conv2d_prepared_bytes")
    ws = guarded.scratch(n_ws, poison=r.poison, name="ws")
    pf_g = guarded.scratch(n_prep, poison=r.poison, name="prepared fwd")
    pd_g = guarded.scratch(n_prep, poison=r.poison, name="prepared dgrad")
    conv.ws, conv.ws_bytes = ws.view, n_ws
    Ho, Wo = conv.Ho, conv.Wo
    pshape = (B, Co, Ho // 2, Wo // 2)
    mask_g = guarded.scratch(conv.pool_mask_bytes(), poison=r.poison, name="packed pool mask" if packed else "pool mask")
    mask = mask_g.view if packed else mask_g.view.view(T.int32).view(*pshape)
    pre = "pool/packed/" if packed else "pool/"
    own = [mask_g, ws, pf_g, pd_g]
    if r.call(pre + "prepare_filters", lambda keep: capi.prepare_filters([conv], [r.w], [r.b], [pf_g.view], [pd_g.view]) or {}, extra=own) is None:
        return
    tag = lambda call, what: f"{pre}{call} [{r.where}] {what}"
    # the composition the fused calls are held to (tests/test_gpu_parity.py): forward_relu + maxpool_forward, maxpool_backward_relu + the
    # plain gradient calls -- on plain buffers: they are the reference here, their own scratch is checked in _plain_calls
    plain = capi.Conv2d(B, Ci, H, W, Co, k, s, pad)
    y, yr = T.empty(r.out_shape, device="cuda"), T.empty(r.out_shape, device="cuda")
    plain.forward_relu(r.x, r.w, r.b, y, yr)
    pooled_ref, mask_ref = capi.maxpool_forward(yr, 2, 2)
    dpool = r.operand("dpool", uniform_pm1(77, pshape))
    marked = (mask_ref | T.where(pooled_ref <= 0, T.full_like(mask_ref, -2 ** 31), T.zeros_like(mask_ref))).to(T.int32)
    dy = capi.maxpool_backward_relu(dpool, mask_ref, pooled_ref, r.out_shape, 2, 2)
    gw_ref, gb_ref = plain.backward_weight(r.x, dy, float(B))
    dx_ref = plain.backward_data(dy, r.w)
    T.cuda.synchronize()
    # ... and the oracle on the same delta (the pool / ReLU decisions are exact operations on the HIP forward tensor)
    xp = np.pad(host(r.x), ((0, 0), (0, 0), (pad, pad), (pad, pad))) if pad else host(r.x)
    gw_o, gb_o, dx_o = O.conv2d_backward(xp, host(dy), host(r.w), s)
    p_o, _ = O.maxpool_forward(O.relu_forward(O.conv2d_forward(xp, host(r.w), host(r.b), s)), 2, 2)

    def fwd(prepared):
        def fn(keep):
            mask_g.refill()
            pooled = r.out(pshape, keep)
            conv.relu_maxpool2_forward(r.x, r.w, r.b, pooled, mask, prepared_fwd=pf_g.view if prepared else None)
            return {"pooled": pooled}
        return fn

    for name, prepared in (("relu_maxpool2_forward", False), ("relu_maxpool2_forward_prepared", True)):
        got = r.call(pre + name, fwd(prepared), extra=own, refill=[ws])
        if got is None:
            continue
        _same(pr, tag(name, "pooled == forward_relu + maxpool"), got["pooled"], host(pooled_ref))
        _close(pr, tag(name, "pooled"), got["pooled"], p_o)
        if packed:
            un = r.call(pre + "pool_mask_unpack", lambda keep: {"mask": conv.pool_mask_unpack(mask, r.out(pshape, keep, dtype=T.int32))}, extra=own, refill=[ws])
            if un is not None:
                _same(pr, tag("pool_mask_unpack", "== the int32 mask"), un["mask"], host(marked))
        else:
            _same(pr, tag(name, "mask == maxpool's + bit 31"), host(mask), host(marked))
    if isinstance(r.results.get(pre + "relu_maxpool2_forward_prepared"), Refused):  # (the mask was poisoned in front of that call: nothing may read it)
        return
    pooled_arg = None if packed else pooled_ref
    if r.place is not None:  # the backward calls' mask and pooled operands between poison of their own (the mask: the bytes the fused forward wrote)
        mask = r.operand("packed pool mask (operand)" if packed else "pool mask (operand)", host(mask))
        pooled_arg = None if packed else r.operand("pooled", host(pooled_ref))

    def wgrad(keep):
        gw, gb = r.out(r.w_shape, keep), r.out(r.w_shape[:1], keep)
        conv.backward_weight_pooled2(r.x, dpool, mask, pooled_arg, float(B), gw, gb)
        return {"gw": gw, "gb": gb}

    def dgrad(prepared):
        def fn(keep):
            dx = r.out(r.x_shape, keep)
            conv.backward_data_pooled2(dpool, mask, pooled_arg, r.w, dx, prepared_dgrad=pd_g.view if prepared else None)
            return {"dx": dx}
        return fn

    lr, scale = 0.05, 0.5
    w_new, b_new = r.w.clone(), r.b.clone()
    capi.sgd_update(w_new.view(-1), gw_ref.view(-1), lr, scale)
    capi.sgd_update(b_new, gb_ref, lr, scale)

    def sgd(keep_previous):
        def fn(keep):
            # (the step re-prepares both filter images: guarded buffers of their own, so that pf_g / pd_g keep the images of r.w)
            pf2 = guarded.scratch(n_prep, poison=r.poison, name="prepared fwd (sgd)")
            pd2 = guarded.scratch(n_prep, poison=r.poison, name="prepared dgrad (sgd)")
            keep += [pf2, pd2]
            gw, gb, w2, b2 = r.out(r.w_shape, keep), r.out(r.w_shape[:1], keep), r.out(r.w_shape, keep), r.out(r.w_shape[:1], keep)
            w2.copy_(r.w)
            b2.copy_(r.b)
            outs = {"gw": gw, "gb": gb, "w": w2, "bias": b2}
            P = capi._ptr
            args = [C.byref(conv.desc), P(r.x), P(dpool), P(mask), P(pooled_arg), P(gw), P(gb), float(B), P(w2), P(b2), lr, scale, P(pf2.view), P(pd2.view)]
            if keep_previous:
                wp, bp = r.out(r.w_shape, keep), r.out(r.w_shape[:1], keep)
                outs.update({"w_previous": wp, "bias_previous": bp})
                capi.check(conv.lib.cnn_conv2d_backward_weight_pooled2_sgd_keep(*args, P(wp), P(bp), P(ws.view), n_ws, capi._stream()),
                           "cnn_conv2d_backward_weight_pooled2_sgd_keep")
            else:
                capi.check(conv.lib.cnn_conv2d_backward_weight_pooled2_sgd(*args, P(ws.view), n_ws, capi._stream()),
                           "cnn_conv2d_backward_weight_pooled2_sgd")
            # the images are usable: forward from the new image == forward with the new raw filters
            y1, y2 = r.out(pshape, keep), r.out(pshape, keep)
            plain.relu_maxpool2_forward(r.x, None, None, y1, None, prepared_fwd=pf2.view)
            plain.relu_maxpool2_forward(r.x, w_new, b_new, y2, None)
            outs.update({"pooled from the new image": y1, "pooled from the new filters": y2})
            return outs
        return fn

    got = r.call(pre + "backward_weight_pooled2", wgrad, extra=own, refill=[ws])
    if got is not None:
        for what, hip, ora in (("gw", gw_ref, gw_o), ("gb", gb_ref, gb_o)):
            _same(pr, tag("backward_weight_pooled2", f"{what} == maxpool_backward_relu + backward_weight"), got[what], host(hip))
            _close(pr, tag("backward_weight_pooled2", what), got[what], ora)
    for name, prepared in (("backward_data_pooled2", False), ("backward_data_pooled2_prepared", True)):
        got = r.call(pre + name, dgrad(prepared), extra=own, refill=[ws])
        if got is not None:
            _same(pr, tag(name, "dx == maxpool_backward_relu + backward_data"), got["dx"], host(dx_ref))
            _close(pr, tag(name, "dx"), got["dx"], dx_o)
    for name, keep_previous in (("backward_weight_pooled2_sgd", False), ("backward_weight_pooled2_sgd_keep", True)):
        got = r.call(pre + name, sgd(keep_previous), extra=own, refill=[ws])
        if got is None:
            continue
        for what, want in (("gw", gw_ref), ("gb", gb_ref), ("w", w_new), ("bias", b_new)):
            _same(pr, tag(name, f"{what} == backward_weight_pooled2 + sgd_update"), got[what], host(want))
        _same(pr, tag(name, "the re-prepared forward image"), got["pooled from the new image"], got["pooled from the new filters"])
        if keep_previous:
            _same(pr, tag(name, "w_previous"), got["w_previous"], host(r.w))
            _same(pr, tag(name, "bias_previous"), got["bias_previous"], host(r.b))


SHORT_CALLS = ("forward", "backward_data", "backward_data_relu", "backward_weight", "backward")


def _short_buffers(r, ref):
    """told_bytes in {full / 2, full / 4, 4096, 256}: a status, or 0 with the oracle's result; nothing beyond told_bytes changes"""
    from cnn_amd import capi

    y_ref, gw_ref, gb_ref, dx_ref, dxm_ref = ref
    lib, d, T = r.lib, r.d, r.T
    P, S = capi._ptr, capi._stream
    div = float(r.case[0])
    for call in SHORT_CALLS:
        full = r.sizes["bwd" if call == "backward" else "ws"]
        for told in sorted({full // 2, full // 4, 4096, 256}):
            if told >= full:
                continue
            g = guarded.scratch(full, told_bytes=told, poison=r.poison, name=f"ws told {told} of {full} bytes")
            keep = []
            wsp = P(g.view)
            if call == "forward":
                outs = {"y": r.out(r.out_shape, keep)}
                rc = lib.cnn_conv2d_forward(d, P(r.x), P(r.w), P(r.b), P(outs["y"]), wsp, told, S())
                want = {"y": y_ref}
            elif call == "backward_data":
                outs = {"dx": r.out(r.x_shape, keep)}
                rc = lib.cnn_conv2d_backward_data(d, P(r.dy), P(r.w), P(outs["dx"]), wsp, told, S())
                want = {"dx": dx_ref}
            elif call == "backward_data_relu":
                outs = {"dx": r.out(r.x_shape, keep)}
                rc = lib.cnn_conv2d_backward_data_relu(d, P(r.dy), P(r.w), P(r.relu_below), P(outs["dx"]), wsp, told, S())
                want = {"dx": dxm_ref}
            else:
                outs = {"gw": r.out(r.w_shape, keep), "gb": r.out(r.w_shape[:1], keep)}
                want = {"gw": gw_ref, "gb": gb_ref}
                if call == "backward_weight":
                    rc = lib.cnn_conv2d_backward_weight(d, P(r.x), P(r.dy), P(outs["gw"]), P(outs["gb"]), div, wsp, told, S())
                else:
                    outs["dx"] = r.out(r.x_shape, keep)
                    want["dx"] = dx_ref
                    rc = lib.cnn_conv2d_backward(d, P(r.x), P(r.dy), P(r.w), P(outs["gw"]), P(outs["gb"]), P(outs["dx"]), div, wsp, told, S(), 0)
            where = f"{call} with {told} of {full} bytes [{r.where}]"
            if rc >= 1000:  # (CNN_AMD_E_HIP: a launch error is no refusal, and nothing more is started on the device)
                pytest.exit(f"HIP error {rc} from {where} of desc {r.case}: {lib.cnn_amd_last_error().decode()}", returncode=3)
            try:
                T.cuda.synchronize()
            except RuntimeError as e:
                pytest.exit(f"device error behind {where} of desc {r.case}: {e}", returncode=3)
            for msg in guarded.check([g] + keep):
                r.problems.append(f"{where} (status {rc}): {msg}")
            if rc == 0:
                for what, t in outs.items():
                    _close(r.problems, f"{where} returned 0: {what}", host(t), want[what])


@pytest.mark.parametrize("param", PARAMS, ids=_id)
def test_conv_calls_live_within_their_scratch(T, param, golden, lib_option):
    from cnn_amd import capi

    case, opts = param
    for name, value in opts:
        lib_option(name, value)
    B, Ci, H, W, Co, k, s, pad = case[:8]
    seed = 9000 + 7 * PARAMS.index(param)
    x, w, b = uniform01(seed, (B, Ci, H, W)), normal_scaled(seed + 1, (Co, Ci, k, k)), normal_scaled(seed + 2, (Co,))
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    dy = uniform_pm1(seed + 3, (B, Co, Ho, Wo))
    relu_below = np.maximum(x - np.float32(0.5), np.float32(0))
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad))) if pad else x
    y_ref = O.conv2d_forward(xp, w, b, s)
    gw_ref, gb_ref, dxp = O.conv2d_backward(xp, dy, w, s)
    dx_ref = dxp[:, :, pad:pad + H, pad:pad + W] if pad else dxp
    ref = (y_ref, gw_ref, gb_ref, dx_ref, np.where(relu_below <= 0, np.float32(0), dx_ref))

    recorded = golden.get(R.key(case), {})
    pinned = recorded if not opts else {}  # (the digests were recorded under the default options)
    # a refusal with full-size buffers is the recorded behaviour of that call of that desc, or the packed-mask flag on a call that carries a
    # plain weight gradient; nothing else may refuse, under a measurement switch either
    flagged = len(case) > 8 and case[8] != 0
    may_refuse = lambda call: ("rc" in recorded.get(call, {}) or
                               (flagged and "backward" in call and "backward_data" not in call and not call.startswith("pool/")))
    problems, runs = [], []
    T.cuda.synchronize()
    capi.kernel_timing(1)
    try:
        for poison in guarded.POISONS:
            r = Run(T, case, poison, (x, w, b, dy, relu_below), problems)
            runs.append(r)
            for name, fn in _plain_calls(r).items():
                r.call(name, fn)
            for g in (r.pf, r.pd):
                g.refill()
            prepared = r.call("prepare_filters", lambda keep: capi.prepare_filters([r.conv], [r.w], [r.b], [r.pf.view], [r.pd.view]) or {})
            if prepared is not None:
                for name, fn in _prepared_calls(r).items():
                    r.call(name, fn)
            _check_conv_results(r, ref, may_refuse)
            if r.conv.relu_maxpool2_supported():
                plain = capi.Conv2d(B, Ci, H, W, Co, k, s, pad)
                _pool_family(r, packed=False)
                if plain.pool_mask_packed_supported():
                    _pool_family(r, packed=True)
                for call, outs in r.results.items():
                    if call.startswith("pool/") and isinstance(outs, Refused) and not may_refuse(call):
                        problems.append(f"{call} [{poison}]: refused with full-size buffers: {outs}")
            _short_buffers(r, ref)
        T.cuda.synchronize()
    finally:
        capi.kernel_timing(0)
    for r in runs:  # the added descs: the stage-1 rows / the split-K partial tensors were really used, by the workspace and by the prepared path
        for call, kernel in MUST_LAUNCH.get(param, {}).items():
            if kernel not in r.logs.get(call, ()):
                problems.append(f"{call} [{r.where}]: no {kernel} launch, the log holds {sorted(r.logs.get(call, ()))}")
    # the same bits under both poisons wherever the route golden pins a digest for that call of that desc (those calls repeat)
    a, b2 = runs[0].results, runs[1].results
    for call, rec in pinned.items():
        if "sha" in rec and isinstance(a.get(call), dict) and isinstance(b2.get(call), dict):
            for what in a[call]:
                _same(problems, f"{call} {what}: NaN poison vs 0x5A poison", a[call][what], b2[call][what])
    assert not problems, f"desc {case} {dict(opts)}: {len(problems)} problem(s)\n  " + "\n  ".join(problems[:40])


# ---- BatchNorm2D -----------------------------------------------------------------------------------------------------------------------
BN_CASES = [BN_SHAPES[0], BN_SHAPES[2], BN_SHAPES[7], POOLED_SHAPES[4]]  # general path, channel-resident path, tiny ragged planes, a pooled shape


@pytest.mark.parametrize("shape", BN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_calls_live_within_their_workspace(T, shape):
    _batchnorm_calls(T, shape)


def _batchnorm_calls(T, shape, guard_operands=False):
    """guard_operands (tests/test_gpu_operand_contract.py): x, gamma, beta, the moving and the saved statistics, dpool, mask and pooled lie
    between the poison of the run too (guarded.operand), and their canaries are asked with the workspace's after every call"""
    from cnn_amd import capi

    L = capi.load()
    B, Cc, H, W = shape
    x = (uniform_pm1(70, shape) * 2 + 0.5).astype(np.float32)
    gamma, beta = (uniform_pm1(71, (Cc,)) + 1.5).astype(np.float32), uniform_pm1(72, (Cc,)).astype(np.float32)
    mm0, mv0 = uniform_pm1(73, (Cc,)).astype(np.float32), (uniform_pm1(74, (Cc,)) + 1.5).astype(np.float32)
    dy = uniform_pm1(75, shape).astype(np.float32)
    y_o, _, sm_o, sv_o, mm_o, mv_o = O.batchnorm_forward(x, gamma, beta, mm0, mv0)
    ye_o = O.batchnorm_forward(x, gamma, beta, mm0, mv0, training=False)[0]
    dx_o, gg_o, gb_o = O.batchnorm_backward(x, dy, gamma, sm_o, sv_o)
    pool_ok = H % 2 == 0 and W % 2 == 0 and bool(L.cnn_batchnorm2d_forward_relu_pool_supported(B, Cc, H, W))
    if shape in POOLED_SHAPES:  # (the shape that is here for the two pooled forms: they must really run)
        assert pool_ok and bool(L.cnn_batchnorm2d_backward_pooled_supported(B, Cc, H, W)), shape
    problems = []
    n_ws = int(L.cnn_batchnorm2d_workspace_bytes(B, Cc, H, W))
    for poison in guarded.POISONS:
        operands = []  # (the guards of the placed operands)
        up = (lambda name, a, poison=poison, operands=operands: guarded.operand(a, poison, operands, name)) if guard_operands else (lambda name, a: dev(T, a))
        xd, gd, bd = up("x", x), up("gamma", gamma), up("beta", beta)
        bn = capi.BatchNorm2d(B, Cc, H, W)
        if guard_operands:
            bn.saved_mean, bn.saved_var = up("saved_mean", np.zeros(Cc, np.float32)), up("saved_var", np.zeros(Cc, np.float32))
        ws = guarded.scratch(n_ws, poison=poison, name="bn ws")
        bn.ws, bn.ws_bytes = ws.view, n_ws
        P = capi._ptr
        wsp = P(ws.view) if n_ws else None

        def call(name, fn):
            ws.refill()
            keep = []
            outs = fn(keep)
            T.cuda.synchronize()
            problems.extend(f"{name} [{poison}]: {m}" for m in guarded.check([ws] + operands + keep))
            return {k_: host(v) for k_, v in outs.items()}

        out = lambda keep, shp=shape, dtype=None: guarded.output(shp, poison, keep, dtype=dtype)
        vec = lambda keep: guarded.output((Cc,), poison, keep)

        def forward(training, relu):
            def fn(keep):
                y, mm, mv = out(keep), up("moving_mean", mm0), up("moving_var", mv0)
                yr = out(keep) if relu else None
                bn.forward(xd, gd, bd, mm, mv, y, training=training, y_relu=yr)
                res = {"y": y, "mm": mm, "mv": mv, "mean": bn.saved_mean.clone(), "var": bn.saved_var.clone()}
                if relu:
                    res["y_relu"] = yr
                return res
            return fn

        def backward(keep):
            dyd, gg, gb = out(keep), vec(keep), vec(keep)
            dyd.copy_(dev(T, dy))
            bn.backward(xd, dyd, gd, gg, gb)
            return {"dx": dyd, "gg": gg, "gb": gb}

        tr = call("forward(train)", forward(True, False))
        for what, want in (("y", y_o), ("mean", sm_o), ("var", sv_o), ("mm", mm_o), ("mv", mv_o)):
            _close(problems, f"forward(train) [{poison}] {what}", tr[what], want)
        trr = call("forward_relu(train)", forward(True, True))
        for what in ("y", "mm", "mv", "mean", "var"):  # (test_batchnorm_train_forward_backward_vs_oracle: y unchanged bit for bit)
            _same(problems, f"forward_relu(train) [{poison}] {what} == forward's", trr[what], tr[what])
        _same(problems, f"forward_relu(train) [{poison}] y_relu == relu(y)", trr["y_relu"], np.where(trr["y"] >= 0, trr["y"], np.float32(0)))
        ev = call("forward(eval)", forward(False, False))
        if not np.array_equal(ev["y"], ye_o) or not np.array_equal(ev["mm"], mm0) or not np.array_equal(ev["mv"], mv0):
            problems.append(f"forward(eval) [{poison}]: not the oracle's bits / moving statistics touched")  # (test_batchnorm_eval_uses_moving_statistics)
        evr = call("forward_relu(eval)", forward(False, True))
        _same(problems, f"forward_relu(eval) [{poison}] y", evr["y"], ev["y"])
        _same(problems, f"forward_relu(eval) [{poison}] y_relu == relu(y)", evr["y_relu"], np.where(evr["y"] >= 0, evr["y"], np.float32(0)))
        call("forward(train) again", forward(True, False))  # (the saved statistics of the batch for the backward passes)
        bw = call("backward", backward)
        for what, want in (("dx", dx_o), ("gg", gg_o), ("gb", gb_o)):
            _close(problems, f"backward [{poison}] {what}", bw[what], want)
        if pool_ok:
            pshape = (B, Cc, H // 2, W // 2)
            rd = dev(T, trr["y_relu"])
            p1, m1 = capi.maxpool_forward(rd, 2, 2)
            if guard_operands:
                p1, m1 = up("pooled", host(p1)), up("mask", host(m1))

            def relu_pool(keep):
                pooled, mask = out(keep, pshape), out(keep, pshape, T.int32)
                y, yr, mm, mv = out(keep), out(keep), up("moving_mean", mm0), up("moving_var", mv0)
                bn.forward_relu_pool(xd, gd, bd, mm, mv, pooled, mask, y=y, y_relu=yr, training=True)
                return {"pooled": pooled, "mask": mask, "y": y, "y_relu": yr, "mm": mm, "mv": mv}

            fp = call("forward_relu_pool", relu_pool)  # (test_batchnorm_relu_maxpool_in_one_apply_pass: the two-call sequence, bit for bit)
            for what, want in (("pooled", host(p1)), ("mask", host(m1)), ("y", trr["y"]), ("y_relu", trr["y_relu"]), ("mm", trr["mm"]), ("mv", trr["mv"])):
                _same(problems, f"forward_relu_pool [{poison}] {what} == forward_relu + maxpool", fp[what], want)
            _close(problems, f"forward_relu_pool [{poison}] pooled", fp["pooled"], O.maxpool_forward(O.relu_forward(y_o), 2, 2)[0])
            if bn.backward_pooled_supported():
                dpool = up("dpool", uniform_pm1(83, pshape))
                d_relu = capi.maxpool_backward_relu(dpool, m1, p1, shape, 2, 2)
                dx3_o, gg3_o, gb3_o = O.batchnorm_backward(x, host(d_relu), gamma, sm_o, sv_o)

                def sep(keep):
                    dyd, gg, gb = out(keep), vec(keep), vec(keep)
                    dyd.copy_(d_relu)
                    bn.backward(xd, dyd, gd, gg, gb)
                    return {"dx": dyd, "gg": gg, "gb": gb}

                def pooled_bwd(keep):
                    dx, gg, gb = out(keep), vec(keep), vec(keep)
                    bn.backward_pooled(xd, dpool, m1, p1, gd, gg, gb, dx)
                    return {"dx": dx, "gg": gg, "gb": gb}

                s3, p3 = call("backward(pool delta)", sep), call("backward_pooled", pooled_bwd)
                for what, want in (("dx", dx3_o), ("gg", gg3_o), ("gb", gb3_o)):
                    _close(problems, f"backward_pooled [{poison}] {what}", p3[what], want)
                    _same(problems, f"backward_pooled [{poison}] {what} == maxpool_backward_relu + backward", p3[what], s3[what])
        # the four sync-BN phases on one rank (the all-reduce of one rank is the identity)
        count, dims = float(B * H * W), (B, Cc, H, W)

        def sync_forward(keep):
            s1, s2, y, mm, mv = vec(keep), vec(keep), out(keep), up("moving_mean", mm0), up("moving_var", mv0)
            capi.check(L.cnn_batchnorm2d_partial_sums(P(xd), None, 0.0, P(s1), *dims, wsp, n_ws, capi._stream()), "partial_sums 1")
            T.cuda.synchronize()
            problems.extend(f"partial_sums(1) [{poison}]: {m}" for m in guarded.check([ws] + operands))
            ws.refill()
            capi.check(L.cnn_batchnorm2d_partial_sums(P(xd), P(s1), count, P(s2), *dims, wsp, n_ws, capi._stream()), "partial_sums 2")
            T.cuda.synchronize()
            problems.extend(f"partial_sums(2) [{poison}]: {m}" for m in guarded.check([ws] + operands))
            ws.refill()
            capi.check(L.cnn_batchnorm2d_forward_from_sums(P(xd), P(y), P(gd), P(bd), P(mm), P(mv), P(bn.saved_mean), P(bn.saved_var), P(s1), P(s2), count,
                                                           *dims, bn.eps, bn.momentum, capi._stream()), "forward_from_sums")
            return {"y": y, "mm": mm, "mv": mv, "mean": bn.saved_mean.clone(), "var": bn.saved_var.clone()}

        def sync_backward(keep):
            s4, dyd, gg, gb = guarded.output((4 * Cc,), poison, keep), out(keep), vec(keep), vec(keep)
            dyd.copy_(dev(T, dy))
            capi.check(L.cnn_batchnorm2d_backward_sums(P(xd), P(dyd), P(gd), P(bn.saved_mean), P(bn.saved_var), P(s4), *dims, bn.eps, wsp, n_ws,
                                                       capi._stream()), "backward_sums")
            T.cuda.synchronize()
            problems.extend(f"backward_sums [{poison}]: {m}" for m in guarded.check([ws] + operands))
            ws.refill()
            capi.check(L.cnn_batchnorm2d_backward_from_sums(P(xd), P(dyd), P(gd), P(bn.saved_mean), P(bn.saved_var), P(s4), count, P(gg), P(gb), *dims,
                                                            bn.eps, capi._stream()), "backward_from_sums")
            return {"dx": dyd, "gg": gg, "gb": gb}

        sf = call("partial_sums + forward_from_sums", sync_forward)
        for what, want in (("y", y_o), ("mean", sm_o), ("var", sv_o), ("mm", mm_o), ("mv", mv_o)):
            _close(problems, f"forward_from_sums [{poison}] {what}", sf[what], want)
        sb = call("backward_sums + backward_from_sums", sync_backward)
        for what, want in (("dx", dx_o), ("gg", gg_o), ("gb", gb_o)):
            _close(problems, f"backward_from_sums [{poison}] {what}", sb[what], want)
    assert not problems, f"BatchNorm2D {shape}: {len(problems)} problem(s)\n  " + "\n  ".join(problems[:40])


# ---- cnn_clip_grad_norm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000, 262145])
def test_clip_grad_norm_lives_within_its_workspace(T, n):
    """compared as tests/test_gpu_adam.py::test_clip_kernel compares: stats[0] the fp64 norm or its fp32 neighbour, the coefficient and the
    scaled gradients ref_clip from the device's own stats[0], bit for bit"""
    from cnn_amd import capi

    lib = capi.load()
    rs = np.random.RandomState(50 + n % 97)
    g = rs.standard_normal(n).astype(np.float32)
    want_total = ref_total_norm(g)
    n_ws = int(lib.cnn_clip_grad_norm_workspace_bytes(n))
    assert n_ws > 0
    problems = []
    for poison in guarded.POISONS:
        ws = guarded.scratch(n_ws, poison=poison, name="clip ws")
        keep = []
        gd, stats = guarded.output((n,), poison, keep), guarded.output((2,), poison, keep)
        gd.copy_(dev(T, g))
        capi.check(lib.cnn_clip_grad_norm(capi._ptr(gd), n, 0.5 * float(want_total), 1.0, capi._ptr(ws.view), n_ws, capi._ptr(stats), capi._stream()),
                   "cnn_clip_grad_norm")
        T.cuda.synchronize()
        problems.extend(f"[{poison}] {m}" for m in guarded.check([ws] + keep))
        st = host(stats)
        apart = abs(int(st[:1].view(np.uint32)[0]) - int(np.asarray([want_total], np.float32).view(np.uint32)[0]))
        if not apart <= 1:
            problems.append(f"[{poison}] total norm {st[0]!r}, fp64 reference {want_total!r}: {apart} ulp apart")
            continue
        want_g, want_coef = ref_clip(g, st[0], 0.5 * float(want_total))
        if not (want_coef < 1 and np.array_equal(bits(st[1:2]), bits(np.asarray([want_coef], np.float32)))):
            problems.append(f"[{poison}] coefficient {st[1]!r}, reference {want_coef!r}")
        _same(problems, f"[{poison}] scaled gradients", host(gd), want_g)
    assert not problems, f"cnn_clip_grad_norm n={n}:\n  " + "\n  ".join(problems)


# ---- cnn_conv2d_autotune_ws ------------------------------------------------------------------------------------------------------------
def test_autotune_lives_within_its_scratch(T):
    """geometries no other test uses (the measured choice is pinned per process); the guards only"""
    from cnn_amd import capi

    lib = capi.load()
    for poison, geometry in zip(guarded.POISONS, [(2, 6, 11, 10, 40, 3, 1, 1), (2, 6, 10, 11, 40, 3, 1, 1)]):  # (measured once per process each)
        d = capi.ConvDesc(*geometry)
        n = int(lib.cnn_conv2d_autotune_workspace_bytes(C.byref(d)))
        assert n > 0, "nothing to measure for this geometry: the test would check nothing"
        g = guarded.scratch(n, poison=poison, name="autotune scratch")
        capi.check(lib.cnn_conv2d_autotune_ws(C.byref(d), capi._ptr(g.view), n, capi._stream()), "cnn_conv2d_autotune_ws")
        T.cuda.synchronize()
        rep = g.intact()
        assert rep, f"{geometry} [{poison}] {rep}"
