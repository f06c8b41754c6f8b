"""The fixed Conv2D descs and the two records behind tests/golden/conv_route_sizes.json and tests/golden/conv_routes.json.

The makers (tests/golden/make_conv_route_sizes.py, make_conv_routes.py) and the tests (test_conv_route_sizes.py,
test_gpu_conv_routes.py) call the SAME functions here, so a golden file and the test that reads it cannot drift apart.  Both files
pin what the host-side dispatch decides -- buffer sizes, capability answers, which kernels a call launches -- and, for the GPU
record, the bytes every call writes; they were recorded with the library of the commit BEFORE the dispatch tables existed
(cnn_amd/csrc/conv_dispatch.hip, the slab-family table of conv_wgrad.hip) and must keep passing across host-side refactors."""
import ctypes as C
import hashlib
import re

import numpy as np

from tests.util import normal_scaled, uniform01, uniform_pm1

PACKED = 1  # CNN_CONV2D_POOL_MASK_PACKED

# (B, Ci, H, W, Co, k, s, pad[, flags]): one or two per kernel family and per boundary between two of them, B <= 3, every plane at the
# smallest size its family covers (224 only for the first-layer kernels)
HAND_PICKED = [
    (2, 3, 224, 224, 16, 3, 2, 0),   # first layer (conv_direct.hip) at the reference size
    (2, 3, 9, 9, 16, 3, 2, 0),       # ... and on a plane smaller than one tile
    (2, 3, 56, 56, 16, 3, 2, 0, PACKED),  # ... with the packed pool mask asked for
    (2, 3, 32, 32, 64, 7, 2, 3),     # the 3 -> 64 7x7 stem (conv_stem.hip forward, conv_dgrad_thin.hip packed data gradient)
    (3, 3, 38, 44, 72, 7, 2, 3),     # ... W % 8 != 0: no stem weight gradient; two channel blocks
    (2, 64, 7, 7, 32, 1, 1, 0),      # 1x1, stride 1 (conv_1x1.hip)
    (3, 32, 9, 11, 48, 1, 2, 0),     # 1x1, stride 2, odd sizes
    (2, 3, 32, 32, 16, 3, 1, 1),     # Ci = 3, stride 1: thin data gradient with scalar operands
    (2, 3, 9, 5, 7, 3, 1, 0),        # ... pad 0, image smaller than a patch
    (2, 16, 55, 55, 32, 3, 2, 0),    # the reference net's stride-2 layers: fwd_rd, pk_s2 data gradient, os / rd weight gradient
    (2, 32, 27, 27, 64, 3, 2, 0),
    (2, 64, 13, 13, 128, 3, 2, 0),
    (2, 32, 7, 7, 64, 3, 1, 1),      # 3x3 stride 1 pad 1 by width: the per-width row-kernel instances ...
    (2, 32, 14, 14, 64, 3, 1, 1),
    (2, 32, 28, 28, 128, 3, 1, 1),
    (2, 16, 56, 56, 32, 3, 1, 1),
    (1, 16, 112, 112, 32, 3, 1, 1),
    (2, 16, 30, 30, 32, 3, 1, 1),    # ... the runtime-width kernel between them ...
    (2, 16, 59, 59, 32, 3, 1, 1),
    (1, 8, 12, 226, 16, 3, 1, 1),    # ... and a width behind its widest class
    (1, 64, 112, 112, 128, 3, 1, 0),  # the north-star shape: 112-wide rows, pad 0
    (3, 32, 9, 11, 64, 3, 1, 0),     # stride-1 register-direct data gradient, one tile
    (2, 64, 8, 7, 128, 3, 1, 0),     # ... two tiles per wave
    (2, 64, 56, 56, 128, 3, 2, 1),   # 3x3 stride 2 pad 1: stage entries of the ResNet-shaped stack
    (2, 16, 28, 28, 40, 3, 2, 1),
    (2, 64, 14, 14, 128, 3, 2, 1),
    (2, 5, 13, 11, 7, 5, 2, 0),      # k = 5: only the implicit GEMM / split-K weight gradient
    (1, 20, 17, 19, 130, 3, 3, 0),   # stride 3, Co not a tile multiple
    (2, 6, 10, 10, 40, 3, 1, 1),     # channels below every specialised family
    (2, 7, 8, 8, 5, 3, 2, 1),
    (2, 16, 21, 23, 24, 3, 2, 0),    # stride 2, Ci = 16, Co no register-direct size: the packed VALU data gradient (pk_s2)
]
# the descs repeated under each option: first layers, the stride-2 reference layers, the stem, a thin layer, rows, 1x1, a stage entry
OPTION_CASES = [HAND_PICKED[i] for i in (0, 1, 2, 3, 6, 7, 9, 10, 11, 13, 15, 23)]
OPTIONS = [("WGRAD_RD", "0"), ("NO_DIRECT", "1"), ("PK_DGRAD", "1")]
# the descs whose forward / data gradient the row kernels serve: run once more with the workspace offset by 4 bytes
ROWS_CASES = HAND_PICKED[12:21] + HAND_PICKED[23:26]


def sweep_cases():
    from tests.test_gpu_parity import _sweep_cases

    return [c for seed in (1, 2, 3) for c in _sweep_cases(40, seed)]


def key(case):
    return ",".join(str(v) for v in case)


def desc(case):
    from cnn_amd import capi

    return capi.ConvDesc(*case[:8], case[8] if len(case) > 8 else 0)


# ---- sizes and predicates (no device needed) ------------------------------------------------------------------------------------
SIZE_FIELDS = ["cnn_conv2d_workspace_bytes", "cnn_conv2d_prepared_bytes", "cnn_conv2d_relu_only_supported",
               "cnn_conv2d_relu_maxpool2_supported", "cnn_conv2d_pool_mask_packed_supported", "cnn_conv2d_pool_mask_bytes"]


def size_record():
    """{"default" | "<OPTION>=<v>": {desc key: [the six SIZE_FIELDS answers]}}"""
    from cnn_amd import capi

    lib = capi.load()

    def ask(cases):
        out = {}
        for c in cases:
            d = desc(c)
            out[key(c)] = [int(getattr(lib, f)(C.byref(d))) for f in SIZE_FIELDS]
        return out

    rec = {"default": ask(sweep_cases() + HAND_PICKED)}
    for name, value in OPTIONS:
        with capi.option(name, value):
            rec[f"{name}={value}"] = ask(OPTION_CASES)
    return rec


# ---- routes and results (GPU) ---------------------------------------------------------------------------------------------------
def _sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


class _Layer:
    """seeded inputs of one desc on the device, and fresh (poisoned) output tensors per call.  inputs = (x, w, b, dy, relu_below) as host
    arrays replaces the seeded ones, divisor the weight gradient's (default: the batch size) -- tests/test_gpu_exact_sums.py"""

    def __init__(self, T, case, seed, inputs=None, divisor=None):
        from cnn_amd import capi

        B, Ci, H, W, Co, k, s, pad = case[:8]
        self.T, self.case = T, case
        self.divisor = float(B if divisor is None else divisor)
        self.conv = capi.Conv2d(B, Ci, H, W, Co, k, s, pad)
        self.conv.desc.flags = case[8] if len(case) > 8 else 0
        Ho, Wo = self.conv.Ho, self.conv.Wo
        dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
        if inputs is not None:
            self.x, self.w, self.b, self.dy, self.relu_below = (dev(a) for a in inputs)
            assert self.x.shape == (B, Ci, H, W) and self.w.shape == (Co, Ci, k, k) and self.b.shape == (Co,)
            assert self.dy.shape == (B, Co, Ho, Wo) and self.relu_below.shape == self.x.shape
            return
        self.x = dev(uniform01(seed, (B, Ci, H, W)))
        self.w = dev(normal_scaled(seed + 1, (Co, Ci, k, k)))
        self.b = dev(normal_scaled(seed + 2, (Co,)))
        self.dy = dev(uniform_pm1(seed + 3, (B, Co, Ho, Wo)))
        self.relu_below = capi.relu_forward(self.x - 0.5)

    def y(self):
        return self.T.full(self.conv.out_shape(), 7.0, dtype=self.T.float32, device="cuda")

    def dx(self):
        return self.T.full_like(self.x, 7.0)


def _logged(T, fn):
    """runs fn() -> {name: tensor} | int error code with the launch log on: {"log": {key: launches}, "sha": {...}} | {"log", "rc"}"""
    out, log = _logged_outputs(T, fn)
    if isinstance(out, int):
        return {"log": log, "rc": out}
    return {"log": log, "sha": {name: _sha(t) for name, t in sorted(out.items())}}


def _logged_outputs(T, fn):
    """... -> ({name: tensor} | int error code, {key: launches})"""
    from cnn_amd import capi

    T.cuda.synchronize()
    capi.kernel_timing(1)
    try:
        try:
            out = fn()
        except capi.CnnAmdError as e:  # (a call the library refuses, e.g. a weight gradient with the packed-mask flag: its code is the record)
            out = int(re.search(r"failed with code (-?\d+)", str(e)).group(1))
        T.cuda.synchronize()
        log = {k: cnt for k, (cnt, _) in capi.kernel_timing_report().items()}
    finally:
        capi.kernel_timing(0)
    return out, log


def _raw(L, mode, ws, ws_bytes):
    """forward / data gradient through plain ctypes with the given workspace (None: withheld): the outputs, or the error code"""
    from cnn_amd import capi

    lib, d = L.conv.lib, C.byref(L.conv.desc)
    wsp = None if ws is None else C.c_void_p(ws)
    if mode == 0:
        y = L.y()
        rc = lib.cnn_conv2d_forward(d, capi._ptr(L.x), capi._ptr(L.w), capi._ptr(L.b), capi._ptr(y), wsp, ws_bytes, capi._stream())
        return {"y": y} if rc == 0 else int(rc)
    dx = L.dx()
    rc = lib.cnn_conv2d_backward_data(d, capi._ptr(L.dy), capi._ptr(L.w), capi._ptr(dx), wsp, ws_bytes, capi._stream())
    return {"dx": dx} if rc == 0 else int(rc)


def _calls(L, offset_ws):
    """name -> thunk of every unprepared call of one layer"""
    conv = L.conv

    def forward_relu():
        y, yr = L.y(), L.y()
        conv.forward_relu(L.x, L.w, L.b, y, yr)
        return {"y": y, "y_relu": yr}

    def backward_weight():
        gw, gb = conv.backward_weight(L.x, L.dy, L.divisor)
        return {"gw": gw, "gb": gb}

    calls = {
        "forward": lambda: {"y": conv.forward(L.x, L.w, L.b, L.y())},
        "forward_relu": forward_relu,
        "backward_data": lambda: {"dx": conv.backward_data(L.dy, L.w, L.dx())},
        "backward_data_relu": lambda: {"dx": conv.backward_data_relu(L.dy, L.w, L.relu_below, L.dx())},
        "backward_weight": backward_weight,
        # the fall-through of routes that need a buffer: rows -> next family, packed thin -> scalar thin, pk_s2 -> implicit GEMM
        "forward/no_ws": lambda: _raw(L, 0, None, 0),
        "backward_data/no_ws": lambda: _raw(L, 1, None, 0),
    }
    if offset_ws:  # a workspace the row kernels cannot use (not 16-byte aligned)
        calls["forward/ws+4"] = lambda: _raw(L, 0, conv.ws.data_ptr() + 4, conv.ws_bytes - 4)
        calls["backward_data/ws+4"] = lambda: _raw(L, 1, conv.ws.data_ptr() + 4, conv.ws_bytes - 4)
    return calls


def _prepared_calls(L, pf, pd):
    conv = L.conv

    def forward_prepared():
        y, yr = L.y(), L.y()
        conv.forward_prepared(L.x, pf, L.b, y, yr)
        return {"y": y, "y_relu": yr}

    return {
        "forward_prepared": forward_prepared,
        "backward_data_prepared": lambda: {"dx": conv.backward_data_prepared(L.dy, pd, L.dx())},
        "backward_data_relu_prepared": lambda: {"dx": conv.backward_data_relu(L.dy, None, L.relu_below, L.dx(), prepared_dgrad=pd)},
    }


def route_record(T, repeats=1):
    """{desc key | "prepare_filters[i]": {call: {"log": ..., "sha" | "rc": ...}}} over HAND_PICKED; repeats > 1 (the maker): every call
    runs that often, and a call whose digests do not repeat keeps its log only -- returns (record, [names of such calls])"""
    from cnn_amd import capi

    rec, unstable = {}, []

    def run(where, name, fn):
        got = [_logged(T, fn) for _ in range(repeats)]
        first = got[0]
        assert all(g["log"] == first["log"] and g.get("rc") == first.get("rc") for g in got), (where, name, got)
        if any(g.get("sha") != first.get("sha") for g in got):
            unstable.append(f"{where}:{name}")
            first = {"log": first["log"]}
        rec.setdefault(where, {})[name] = first

    layers = [_Layer(T, c, 9000 + 10 * i) for i, c in enumerate(HAND_PICKED)]
    for L in layers:
        for name, fn in _calls(L, L.case in ROWS_CASES).items():
            run(key(L.case), name, fn)
    for g in range(0, len(layers), 6):  # one cnn_conv2d_prepare_filters call over up to six layers
        group = layers[g:g + 6]
        bufs = [L.conv.prepared_buffers() for L in group]
        fwd, dgrad = [b[0] for b in bufs], [b[1] for b in bufs]
        for b in fwd + dgrad:
            b.fill_(0x5A)
        run(f"prepare_filters[{g // 6}]", "prepare_filters",
            lambda: capi.prepare_filters([L.conv for L in group], [L.w for L in group], [L.b for L in group], fwd, dgrad) or {})
        for L, pf, pd in zip(group, fwd, dgrad):
            for name, fn in _prepared_calls(L, pf, pd).items():
                run(key(L.case), name, fn)
    return rec, unstable
