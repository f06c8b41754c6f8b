"""The depthwise calls of the C ABI on guarded buffers (tests/guarded.py), for tests/test_gpu_depthwise.py and
tests/test_gpu_stream_order_depthwise.py: every operand and output lies between NaN guard bands, the workspace is NaN-filled scratch of
exactly the size the query names, and shift_bytes moves x, dy and w off every 16-byte boundary (`shifts`: every operand group by itself)."""
import ctypes as C

import numpy as np

from tests import guarded


class Layer:
    """one case (B, C, H, W, k, s, pad) with its operands (x, w [C][1][k][k], b, dy, relu_below as host arrays) on the device"""

    def __init__(self, T, case, ins, shift_bytes=0, guard_outputs=True, shifts=None):
        """shifts: bytes off the 256-byte boundary per operand group, {"x", "dy", "w", "below", "out"} (out: every output tensor);
        missing groups, and shifts=None, follow shift_bytes: x, dy and w moved by it, relu_below and the outputs on the boundary"""
        from cnn_amd import capi

        B, Cn, H, W, k, s, pad = case
        self.T, self.case, self.lib, self.keep, self.guard_outputs = T, case, capi.load(), [], guard_outputs
        self.desc = capi.ConvDesc(B, Cn, H, W, Cn, k, s, pad, capi.DEPTHWISE)
        self.Ho, self.Wo = capi.conv_out_dim(H, k, s, pad), capi.conv_out_dim(W, k, s, pad)
        x, w, b, dy, below = ins
        sh = dict({"x": shift_bytes, "dy": shift_bytes, "w": shift_bytes, "below": 0, "out": 0}, **(shifts or {}))
        assert set(sh) == {"x", "dy", "w", "below", "out"} and (guard_outputs or sh["out"] == 0), sh
        self.shifts = sh
        op = lambda a, name, by: guarded.operand(np.array(a), keep=self.keep, name=name, shift_bytes=by)
        self.x, self.w, self.dy = op(x, "x", sh["x"]), op(w, "w", sh["w"]), op(dy, "dy", sh["dy"])
        self.b, self.below = op(b, "bias", 0), op(below, "relu_below", sh["below"])
        self.ws_bytes = int(self.lib.cnn_conv2d_workspace_bytes(C.byref(self.desc)))
        self.bws_bytes = int(self.lib.cnn_conv2d_backward_workspace_bytes(C.byref(self.desc)))
        assert 0 < self.ws_bytes <= self.bws_bytes, self.lib.cnn_amd_last_error().decode()
        self.ws = guarded.scratch(self.bws_bytes, name="workspace")
        self.keep.append(self.ws)

    # ---- plumbing ----
    def _s(self):
        from cnn_amd import capi

        return capi._stream()  # torch's current stream

    def _out(self, shape, name):
        if not self.guard_outputs:  # (the stream-order harness: a guarded output is a fresh 128 KiB+ allocation, which waits for the gate)
            return self.T.full(shape, 7.0, dtype=self.T.float32, device="cuda")
        return guarded.output(shape, keep=self.keep, name=name, shift_bytes=self.shifts["out"])

    def _d(self):
        return C.byref(self.desc)

    def y_shape(self):
        B, Cn = self.case[:2]
        return (B, Cn, self.Ho, self.Wo)

    def _ok(self, rc, what):
        from cnn_amd import capi

        capi.check(rc, what)

    def intact(self):
        return guarded.check(self.keep)

    # ---- the calls: each -> {name: tensor} ----
    def forward(self):
        from cnn_amd.capi import _ptr

        y = self._out(self.y_shape(), "y")
        self._ok(self.lib.cnn_conv2d_forward(self._d(), _ptr(self.x), _ptr(self.w), _ptr(self.b), _ptr(y), _ptr(self.ws.view), self.ws_bytes,
                                            self._s()), "cnn_conv2d_forward")
        return {"y": y}

    def forward_relu(self, with_y=True):
        from cnn_amd.capi import _ptr

        y = self._out(self.y_shape(), "y") if with_y else None
        yr = self._out(self.y_shape(), "y_relu")
        self._ok(self.lib.cnn_conv2d_forward_relu(self._d(), _ptr(self.x), _ptr(self.w), _ptr(self.b), _ptr(y), _ptr(yr), _ptr(self.ws.view),
                                                 self.ws_bytes, self._s()), "cnn_conv2d_forward_relu")
        return {"y": y, "y_relu": yr} if with_y else {"y_relu": yr}

    def backward_data(self):
        from cnn_amd.capi import _ptr

        dx = self._out(tuple(self.x.shape), "dx")
        self._ok(self.lib.cnn_conv2d_backward_data(self._d(), _ptr(self.dy), _ptr(self.w), _ptr(dx), _ptr(self.ws.view), self.ws_bytes, self._s()),
                 "cnn_conv2d_backward_data")
        return {"dx": dx}

    def backward_data_relu(self):
        from cnn_amd.capi import _ptr

        dx = self._out(tuple(self.x.shape), "dx_masked")
        self._ok(self.lib.cnn_conv2d_backward_data_relu(self._d(), _ptr(self.dy), _ptr(self.w), _ptr(self.below), _ptr(dx), _ptr(self.ws.view),
                                                       self.ws_bytes, self._s()), "cnn_conv2d_backward_data_relu")
        return {"dx_masked": dx}

    def _grads(self):
        return self._out(tuple(self.w.shape), "gw"), self._out(tuple(self.b.shape), "gb")

    def backward_weight(self, divisor, side=False):
        from cnn_amd.capi import _ptr

        gw, gb = self._grads()
        self.ws.refill()
        fn = self.lib.cnn_conv2d_backward_weight_side if side else self.lib.cnn_conv2d_backward_weight
        self._ok(fn(self._d(), _ptr(self.x), _ptr(self.dy), _ptr(gw), _ptr(gb), float(divisor), _ptr(self.ws.view), self.ws_bytes, self._s()),
                 "cnn_conv2d_backward_weight")
        if side:
            self._ok(self.lib.cnn_amd_side_stream_join(self._s()), "cnn_amd_side_stream_join")
        return {"gw": gw, "gb": gb}

    def backward(self, divisor, defer_join):
        from cnn_amd.capi import _ptr

        gw, gb = self._grads()
        dx = self._out(tuple(self.x.shape), "dx")
        self.ws.refill()
        self._ok(self.lib.cnn_conv2d_backward(self._d(), _ptr(self.x), _ptr(self.dy), _ptr(self.w), _ptr(gw), _ptr(gb), _ptr(dx), float(divisor),
                                             _ptr(self.ws.view), self.bws_bytes, self._s(), int(defer_join)), "cnn_conv2d_backward")
        if defer_join:
            self._ok(self.lib.cnn_amd_side_stream_join(self._s()), "cnn_amd_side_stream_join")
        return {"gw": gw, "gb": gb, "dx": dx}


def logged(T, fn, keys=False):
    """fn() with the kernel-timing report on -> (its result, [kernel names in first-launch order]); keys=True: the whole keys
    "name|geometry tag" instead of the names"""
    from cnn_amd import capi

    T.cuda.synchronize()
    capi.kernel_timing(1)
    try:
        out = fn()
        T.cuda.synchronize()
        names = [k if keys else k.split("|")[0] for k in capi.kernel_timing_report()]
    finally:
        capi.kernel_timing(0)
    return out, names


def host(t):
    return t.detach().cpu().numpy()
