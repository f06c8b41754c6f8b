"""Stream order of the Conv2D entry points (tests/stream_order.py is the harness): the harness's own controls, every call of
tests/conv_route_cases.py caller late against the digests of tests/golden/conv_routes.json, the fork / join family in both placements
against the CPU oracle, and the published kernels with a gated producer."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import conv_route_cases as R
from tests import stream_order as SO
from tests import stream_order_cases as K
from tests.util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture
def H(T):
    h = SO.harness(T)
    try:
        yield h
    finally:
        h.finish()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "conv_routes.json")))


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- controls: pure torch, no library call except the gate itself ------------------------------------------------------------------
def test_control_other_streams_run_beside_a_gated_test_stream(T, H):
    """with S gated, an op on the default stream and one on the library's side stream complete while the gate is live, and with the
    side stream gated one on S does: two streams on one hardware queue fail here, loudly, instead of every case passing without power"""
    assert H.user_streams <= 3
    assert H.runs_beside(H.S, H.default), "the default stream waits for the gated test stream"
    assert H.runs_beside(H.S, H.side), "the side stream waits for the gated test stream"
    assert H.runs_beside(H.side, H.S), "the test stream waits for the gated side stream"
    assert H.runs_beside(H.S, H.S2), "the second stream waits for the gated test stream"


def test_control_a_step_on_the_wrong_stream_is_flagged(T, H):
    """a stand-in "call" of two steps, y = (2 x) + 1: in order on S it passes caller late; with its second step on the default
    stream -- unordered against S -- the comparison fails"""
    x = T.zeros(4096, device="cuda")
    t = T.zeros(4096, device="cuda")  # the stand-in's "workspace": poisoned like one, or the ungated run's product would still lie there
    real = dev(T, K.published_relu_inputs()["x"].repeat(4)[:4096])
    late = [H.late(x, 7401, real)]
    want = real.cpu().numpy() * np.float32(2) + np.float32(1)

    def standin(second):
        def call():
            y = T.full_like(x, 7.0)
            T.mul(x, 2, out=t)
            with T.cuda.stream(second if second is not None else T.cuda.current_stream()):
                T.add(t, 1, out=y)
            return {"y": y}
        return call

    good = H.caller_late("control: in order", late, standin(None), poison=[t])
    assert np.array_equal(good.gated["y"], want)
    bad = H.caller_late("control: second step on the default stream", late, standin(H.default), poison=[t])
    assert not np.array_equal(bad.gated["y"], want)


def test_control_a_missing_join_is_flagged(T, H):
    """a stand-in that forks y = x + 1 onto the side stream: with the join (S waits for the side stream) it passes helper late,
    without it the clone holds the 7.0 fill"""
    x = dev(T, K.published_relu_inputs()["x"])
    want = x.cpu().numpy() + np.float32(1)

    def standin(join):
        def call():
            S = T.cuda.current_stream()
            y = T.full_like(x, 7.0)
            H.side.wait_stream(S)
            with T.cuda.stream(H.side):
                T.add(x, 1, out=y)
            if join:
                S.wait_stream(H.side)
            return {"y": y}
        return call

    good = H.helper_late("control: joined", standin(True))
    assert np.array_equal(good.gated["y"], want)
    bad = H.helper_late("control: no join", standin(False))
    assert np.array_equal(bad.gated["y"], np.full_like(want, 7.0))


def test_control_a_consumer_that_does_not_wait_is_flagged(T, H):
    """the shape of the published-kernel and event cases: a producer on S (gated, input late) writes y = x + 1, a consumer on a
    second stream clones y.  With the wait (S2 waits for an event behind the producer) it passes; without it the consumer runs while S
    is gated and clones the poison -- not the bytes the ungated run left in y"""
    x = T.zeros(4096, device="cuda")
    y = T.empty_like(x)
    real = dev(T, K.published_relu_inputs()["x"].repeat(4)[:4096])
    late = [H.late(x, 7402, real)]
    want = real.cpu().numpy() + np.float32(1)

    def standin(wait):
        def call():
            S = T.cuda.current_stream()
            y.fill_(7.0)
            T.add(x, 1, out=y)
            if wait:
                H.S2.wait_stream(S)
            with T.cuda.stream(H.S2):
                got = y.clone()
            S.wait_stream(H.S2)
            return {"y": got}
        return call

    good = H.caller_late("control: consumer waits", late, standin(True), poison=[y])
    assert np.array_equal(good.gated["y"], want)
    bad = H.caller_late("control: consumer does not wait", late, standin(False), poison=[y])
    assert not np.array_equal(bad.gated["y"], want)
    assert np.isnan(bad.gated["y"]).all(), "the consumer that did not wait saw something else than the poison"


# ---- conv routes, caller late --------------------------------------------------------------------------------------------------------
def _check_golden(res, want, what):
    if "rc" in want:
        assert res.gated == want["rc"], (what, res.gated, want["rc"])
    else:
        assert "sha" in want, what  # (every record of conv_routes.json holds digests or an error code)
        assert not isinstance(res.gated, int), (what, res.gated)
        got = {name: SO.sha(a) for name, a in sorted(res.gated.items())}
        assert got == want["sha"], f"{what}: the gated call's bytes are not the recorded ones"
    res.assert_same_bits_as_plain(what)


def _layer(T, H, i):
    """the layer of HAND_PICKED[i] with the recorder's seed, and its inputs as late operands"""
    case = R.HAND_PICKED[i]
    L = R._Layer(T, case, 9000 + 10 * i)
    T.cuda.synchronize()
    late = {name: H.late(getattr(L, name), 9500 + 10 * i + j) for j, name in enumerate(("x", "w", "b", "dy", "relu_below"))}
    return L, late


@pytest.mark.parametrize("i", range(len(R.HAND_PICKED)), ids=[R.key(c) for c in R.HAND_PICKED])
def test_conv_route_calls_caller_late(T, H, golden, i):
    """every unprepared call of one desc (tests/conv_route_cases.py::_calls) with x, w, bias, dy and relu_below arriving late on S and
    the layer's workspace poisoned: the bytes recorded in tests/golden/conv_routes.json, or the recorded error code"""
    L, late = _layer(T, H, i)
    case = L.case
    for name, fn in R._calls(L, case in R.ROWS_CASES).items():
        res = H.caller_late(f"{R.key(case)}:{name}", list(late.values()), fn, poison=[L.conv.ws])
        _check_golden(res, golden[R.key(case)][name], f"{R.key(case)}:{name}")


@pytest.mark.parametrize("g", range(0, len(R.HAND_PICKED), 6))
def test_prepared_calls_caller_late(T, H, golden, g):
    """cnn_conv2d_prepare_filters over six layers with every w and bias arriving late, then the prepared calls of each layer with
    x / dy / relu_below / bias AND the prepared images of the gated prepare call arriving late: the recorded bytes.  (The record
    holds no digest of the images themselves: the prepared calls that consume them are their check.)"""
    from cnn_amd import capi

    layers = [_layer(T, H, i) for i in range(g, min(g + 6, len(R.HAND_PICKED)))]
    bufs = [L.conv.prepared_buffers() for L, _ in layers]
    fwd, dgrad = [b[0] for b in bufs], [b[1] for b in bufs]

    def prepare():
        for b in fwd + dgrad:
            b.fill_(0x5A)
        capi.prepare_filters([L.conv for L, _ in layers], [L.w for L, _ in layers], [L.b for L, _ in layers], fwd, dgrad)
        return {f"{kind}{j}": b for kind, group in (("fwd", fwd), ("dgrad", dgrad)) for j, b in enumerate(group)}

    late_wb = [late[n] for _, late in layers for n in ("w", "b")]
    prepared = H.caller_late(f"prepare_filters[{g // 6}]", late_wb, prepare)
    prepared.assert_same_bits_as_plain(f"prepare_filters[{g // 6}]")
    assert golden[f"prepare_filters[{g // 6}]"]["prepare_filters"]["sha"] == {}
    for j, (L, late) in enumerate(layers):
        pf, pd = fwd[j], dgrad[j]
        late_p = [H.late(pf, 0, dev(T, prepared.gated[f"fwd{j}"])), H.late(pd, 0, dev(T, prepared.gated[f"dgrad{j}"]))]
        for name, fn in R._prepared_calls(L, pf, pd).items():
            res = H.caller_late(f"{R.key(L.case)}:{name}", list(late.values()) + late_p, fn)
            _check_golden(res, golden[R.key(L.case)][name], f"{R.key(L.case)}:{name}")


# ---- fork and join -------------------------------------------------------------------------------------------------------------------
_fork_refs = {}


def _fork_reference(case, variant):
    """computed once per (desc, kind of reference), shared by both placements"""
    kind = "pooled2" if variant.startswith("pooled2") else "relu" if variant.startswith("prepared_relu") else "plain"
    if (case, kind) not in _fork_refs:
        _fork_refs[(case, kind)] = K.fork_reference(case, {"pooled2": "pooled2", "relu": "prepared_relu", "plain": "backward"}[kind],
                                                    K.fork_inputs(case))
    ref = dict(_fork_refs[(case, kind)])
    if variant == "weight_side_join":
        del ref["dx"]
    return ref


class _Fork:
    """the device side of one fork / join case"""

    def __init__(self, T, H, case, variant):
        from cnn_amd import capi

        self.T, self.H, self.case, self.variant, self.capi = T, H, case, variant, capi
        self.conv = capi.Conv2d(*case)
        self.lib = self.conv.lib
        inp = K.fork_inputs(case)
        self.t = {name: dev(T, a) for name, a in inp.items()}
        bias = self.t.get("bias", T.zeros(case[4], device="cuda"))
        _, self.t["pd"] = self.conv.prepared_buffers()
        capi.prepare_filters([self.conv], [self.t["w"]], [bias], None, [self.t["pd"]])
        nb = int(self.lib.cnn_conv2d_backward_workspace_bytes(C.byref(self.conv.desc)))
        self.bwd_ws = T.empty(nb, dtype=T.uint8, device="cuda")
        T.cuda.synchronize()
        self.reads = K.FORK_VARIANTS[variant]

    def late(self):
        seed = K.fork_seed(self.case) + 50
        return [self.H.late(self.t[name], seed + j) for j, name in enumerate(self.reads)]

    def poison(self):
        return [self.conv.ws, self.bwd_ws]

    def call(self):
        """runs on the current stream: the call, the join its contract names, -> the outputs"""
        T, capi, lib, t, v = self.T, self.capi, self.lib, self.t, self.variant
        conv, d = self.conv, C.byref(self.conv.desc)
        B = float(self.case[0])
        p = capi._ptr
        gw, gb, dx = T.full_like(t["w"], 7.0), T.full((self.case[4],), 7.0, device="cuda"), T.full_like(t["x"], 7.0)
        defer = 1 if "deferred" in v else 0
        ws, ws_bytes = p(conv.ws), conv.ws_bytes
        if v.startswith("backward"):
            capi.check(lib.cnn_conv2d_backward(d, p(t["x"]), p(t["dy"]), p(t["w"]), p(gw), p(gb), p(dx), B, p(self.bwd_ws),
                                               self.bwd_ws.numel(), capi._stream(), defer), "cnn_conv2d_backward")
        elif v == "weight_side_join":
            capi.check(lib.cnn_conv2d_backward_weight_side(d, p(t["x"]), p(t["dy"]), p(gw), p(gb), B, ws, ws_bytes, capi._stream()),
                       "cnn_conv2d_backward_weight_side")
            defer = 1
        elif v.startswith("prepared_relu"):
            capi.check(lib.cnn_conv2d_backward_prepared_relu(d, p(t["x"]), p(t["dy"]), p(t["pd"]), p(t["relu_below"]), p(gw), p(gb), p(dx),
                                                             B, ws, ws_bytes, capi._stream(), defer), "cnn_conv2d_backward_prepared_relu")
        elif v.startswith("prepared"):
            capi.check(lib.cnn_conv2d_backward_prepared(d, p(t["x"]), p(t["dy"]), p(t["pd"]), p(gw), p(gb), p(dx), B, ws, ws_bytes,
                                                        capi._stream(), defer), "cnn_conv2d_backward_prepared")
        else:
            assert v.startswith("pooled2")
            conv.backward_pooled2_prepared(t["x"], t["dpool"], t["mask"], t["pooled"], t["pd"], B, gw, gb, dx, defer_join=bool(defer))
        out = {"gw": gw, "gb": gb}
        if v != "weight_side_join":
            out["dx"] = dx.clone()  # ordered on the caller's stream when the call returns, whatever defer_join says
        if defer:
            if "flush" in v:
                with T.cuda.stream(self.H.side):
                    capi.flush_reduces()
            capi.side_stream_join()
        return out


@pytest.mark.parametrize("placement", ["caller_late", "helper_late"])
@pytest.mark.parametrize("case,variant", K.fork_cases(), ids=[f"{R.key(c)}-{v}" for c, v in K.fork_cases()])
def test_fork_and_join(T, H, case, variant, placement):
    """cnn_conv2d_backward under both defer_join values, cnn_conv2d_backward_weight_side, cnn_amd_flush_reduces on the side stream, the
    prepared forms and the pool-fused one, each followed by cnn_amd_side_stream_join where its contract names it.  Caller late: the
    fork has to wait for the inputs that arrive on S.  Helper late: the side stream is gated, the clones on S have to wait for the
    join.  Reference: the CPU oracle at REL_TOL, as tests/test_gpu_parity.py holds these calls"""
    F = _Fork(T, H, case, variant)
    what = f"{R.key(case)} {variant} {placement}"
    if placement == "caller_late":
        res = H.caller_late(what, F.late(), F.call, poison=F.poison())
    else:
        res = H.helper_late(what, F.call, poison=F.poison())
    ref = _fork_reference(case, variant)
    assert sorted(res.gated) == sorted(ref), what
    for name, want in ref.items():
        assert_close(res.gated[name], want, REL_TOL, f"{what}: {name}")
    res.assert_same_bits_as_plain(what)


# ---- published kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear_backward", "relu", "conv_backward_fork_point"])
def test_published_kernels(T, H, kind):
    """cnn_amd_publish_next_kernel / cnn_amd_wait_published with the producer gated on S and its inputs late: a second stream waits
    through cnn_amd_wait_published and clones the result -- a launch_pub site (linear backward + ReLU', B = 4, 64 -> 3), the fallback
    record (ReLU), and cnn_conv2d_backward taking a published kernel (the ReLU that produces its dy) as its fork point"""
    from cnn_amd import capi

    S2 = H.S2
    if kind == "conv_backward_fork_point":
        case = K.FORK_DESCS[1]
        F = _Fork(T, H, case, "backward_join_now")
        pre = dev(T, K.fork_inputs(case)["dy"])  # dy = relu(pre): the published producer in front of the backward call
        # (dy is written by the published kernel; it is a late operand all the same, so that it holds a decoy until then and not
        # what the ungated run left there)
        late = [H.late(pre, 7391), H.late(F.t["x"], 7392), H.late(F.t["w"], 7393), H.late(F.t["dy"], 7394)]
        inp = K.fork_inputs(case)
        inp["dy"] = K.published_relu_reference({"x": inp["dy"]})["y"]
        ref = K.fork_reference(case, "backward", inp)

        def call():
            # (the inputs that arrive late are queued in front of the published kernel: it is the last thing on S the weight
            # gradient depends on, as the contract of the fork point asks)
            capi.publish_next_kernel()
            capi.relu_forward(pre, F.t["dy"])
            return F.call()

        res = H.caller_late("published: conv backward fork point", late, call, poison=F.poison())
    else:
        if kind == "linear_backward":
            inp, ref = K.published_linear_inputs(), K.published_linear_reference(K.published_linear_inputs())
        else:
            inp, ref = K.published_relu_inputs(), K.published_relu_reference(K.published_relu_inputs())
        t = {name: dev(T, a) for name, a in inp.items()}
        late = [H.late(t[name], 7380 + j) for j, name in enumerate(sorted(t))]
        # The producer's outputs live outside the call and are poisoned in front of the gate: a consumer that does not wait reads
        # them while S is still gated, and must not find there what the ungated run computed.
        out = {"y": T.empty_like(t["x"])} if kind == "relu" else {"gw": T.empty_like(t["w"]), "gb": T.empty(3, device="cuda"), "dx": T.empty_like(t["x"])}

        def call():
            for o in out.values():
                o.fill_(7.0)
            capi.publish_next_kernel()
            if kind == "relu":
                capi.relu_forward(t["x"], out["y"])
            else:
                capi.linear_backward(t["x"], t["dy"], t["w"], 4.0, out["gw"], out["gb"], out["dx"], relu_below=True)
            capi.wait_published(S2)
            with T.cuda.stream(S2):  # (the consumer: ordered behind the producer by the published event alone)
                got = {name: o.clone() for name, o in out.items()}
            T.cuda.current_stream().wait_stream(S2)  # the harness clones and waits on S
            return got

        res = H.caller_late(f"published: {kind}", late, call, poison=list(out.values()))
    assert sorted(res.gated) == sorted(ref)
    for name, want in ref.items():
        assert_close(res.gated[name], want, REL_TOL, f"published {kind}: {name}")
    res.assert_same_bits_as_plain(f"published {kind}")


# ---- the first block's own entry points, the im2col fallback, the tile measurement ------------------------------------------------------
@pytest.mark.parametrize("entry", ["relu_maxpool2_forward", "relu_maxpool2_forward_packed_unpack", "backward_weight_pooled2", "backward_data_pooled2"])
def test_first_block_calls_caller_late(T, H, entry):
    """cnn_conv2d_relu_maxpool2_forward with the int32 mask and with the packed one through cnn_conv2d_pool_mask_unpack,
    cnn_conv2d_backward_weight_pooled2 and cnn_conv2d_backward_data_pooled2 at (2,3,56,56,16,3,2,0), operands late, against the CPU
    oracle at REL_TOL; a mask is held through the ReLU values it points at (an index comparison would fail on a last-bit tie)"""
    from cnn_amd import capi

    case = K.POOLED_DESC
    inp = K.fork_inputs(case)
    conv = capi.Conv2d(*case)
    assert conv.relu_maxpool2_supported()
    t = {name: dev(T, a) for name, a in inp.items()}
    T.cuda.synchronize()
    pshape = inp["pooled"].shape
    f7 = lambda like: T.full_like(like, 7.0)
    if entry.startswith("relu_maxpool2_forward"):
        packed = entry.endswith("packed_unpack")
        if packed:
            assert conv.pool_mask_packed_supported()
            conv.set_pool_mask_packed()
        reads = ("x", "w", "bias")

        def call():
            pooled = f7(t["pooled"])
            mask = T.full(pshape, 7, dtype=T.int32, device="cuda")
            if packed:
                raw = T.full((conv.pool_mask_bytes(),), 7, dtype=T.uint8, device="cuda")
                conv.relu_maxpool2_forward(t["x"], t["w"], t["bias"], pooled, raw)
                conv.pool_mask_unpack(raw, mask)
            else:
                conv.relu_maxpool2_forward(t["x"], t["w"], t["bias"], pooled, mask)
            return {"pooled": pooled, "mask": mask}
    elif entry == "backward_weight_pooled2":
        reads = ("x", "dpool", "mask", "pooled")

        def call():
            gw, gb = f7(t["w"]), f7(t["bias"])
            conv.backward_weight_pooled2(t["x"], t["dpool"], t["mask"], t["pooled"], float(case[0]), gw, gb)
            return {"gw": gw, "gb": gb}
    else:
        reads = ("dpool", "mask", "pooled", "w")
        call = lambda: {"dx": conv.backward_data_pooled2(t["dpool"], t["mask"], t["pooled"], t["w"], f7(t["x"]))}
    late = [H.late(t[name], 7450 + j) for j, name in enumerate(reads)]
    res = H.caller_late("first block " + entry, late, call, poison=[conv.ws])
    if entry.startswith("relu_maxpool2_forward"):
        ref = K.first_block_forward_reference(inp)
        assert_close(res.gated["pooled"], ref["pooled"], REL_TOL, f"{entry}: pooled")
        assert_close(K.pooled_by_mask(ref["relu"], res.gated["mask"]), ref["pooled"], REL_TOL, f"{entry}: the ReLU output where the mask points")
    else:
        ref = K.fork_reference(case, "pooled2", inp)
        for name in res.gated:
            assert_close(res.gated[name], ref[name], REL_TOL, f"{entry}: {name}")
    res.assert_same_bits_as_plain(entry)


@pytest.mark.parametrize("entry", ["forward_im2col", "backward_weight_im2col", "backward_data_im2col"])
def test_im2col_fallback_caller_late(T, H, entry):
    from cnn_amd import capi

    inp = K.im2col_inputs()
    conv = capi.Conv2d(*K.IM2COL_DESC)
    t = {name: dev(T, a) for name, a in inp.items()}
    conv._iws("cuda")  # (the fallback's workspace, allocated on first use: poisoned like any other)
    T.cuda.synchronize()
    late = [H.late(t[name], 7460 + j) for j, name in enumerate(("x", "w", "bias", "dy"))]
    if entry == "forward_im2col":
        call = lambda: {"y": conv.forward_im2col(t["x"], t["w"], t["bias"])}
    elif entry == "backward_weight_im2col":
        call = lambda: dict(zip(("gw", "gb"), conv.backward_weight_im2col(t["x"], t["dy"], float(K.IM2COL_DESC[0]))))
    else:
        call = lambda: {"dx": conv.backward_data_im2col(t["dy"], t["w"])}
    res = H.caller_late(entry, late, call, poison=[conv._im2col_ws])
    ref = K.im2col_reference(inp)
    for name in res.gated:
        assert_close(res.gated[name], ref[name], REL_TOL, f"{entry}: {name}")
    res.assert_same_bits_as_plain(entry)


_tune_co = iter(K.TUNE_CO)


@pytest.mark.parametrize("entry", ["autotune", "autotune_ws"])
def test_tile_measurement_caller_late(T, H, lib_option, entry):
    """cnn_conv2d_autotune / cnn_conv2d_autotune_ws synchronise by contract (liveness is asserted in front of them): with S gated
    and the layer's operands late, S is idle when the call returns, and the forward pass with the tile it pinned equals the CPU
    oracle.  A geometry is measured once per process: every run takes the next Co of tests/stream_order_cases.py::TUNE_CO"""
    from cnn_amd import capi

    lib_option("IGEMM_AUTOTUNE", None)
    lib = capi.load()
    B, Ci, Hh, Ww, k, s, pad = K.TUNE_SHAPE
    inp = K.tune_inputs()
    t = {name: dev(T, a) for name, a in inp.items()}
    T.cuda.synchronize()
    late = [H.late(t[name], 7470 + j) for j, name in enumerate(("x", "w", "bias"))]
    used = []

    def call():
        co = next(_tune_co)
        used.append(co)
        conv = capi.Conv2d(B, Ci, Hh, Ww, co, k, s, pad)
        H.keep.append(conv)
        d = C.byref(conv.desc)
        need = int(lib.cnn_conv2d_autotune_workspace_bytes(d))
        assert need > 0, "the geometry was measured before"
        if entry == "autotune":
            capi.check(lib.cnn_conv2d_autotune(d, capi._stream()), "cnn_conv2d_autotune")
        else:
            scratch = T.empty(need, dtype=T.uint8, device="cuda")
            H.keep.append(scratch)
            capi.check(lib.cnn_conv2d_autotune_ws(d, capi._ptr(scratch), need, capi._stream()), "cnn_conv2d_autotune_ws")
        assert T.cuda.current_stream().query(), "the measurement returned with work pending on its stream"
        assert int(lib.cnn_conv2d_autotune_workspace_bytes(d)) == 0  # measured and pinned
        y = T.full(conv.out_shape(), 7.0, device="cuda")
        return {"y": conv.forward(t["x"], t["w"][:co].contiguous(), t["bias"][:co].contiguous(), y)}

    res = H.caller_late(entry, late, call, blocks=True)
    assert_close(res.gated["y"], K.tune_reference(inp, used[-1])["y"], REL_TOL, f"{entry}: forward with the measured tile")
