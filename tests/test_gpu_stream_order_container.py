"""Stream order of the C++ container on a caller's stream (tests/stream_order.py is the harness): cnnh_set_stream(S) puts every layer
of cnn_amd/host on S -- what bench.py --main-priority does -- and the device-step sequences of tests/host_layer_cases.py run there with
the batch and the labels arriving late, once with S gated and once more with the thread's side stream gated as well, against the
digests of tests/golden/host_layer_traces.json."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from tests import host_layer_cases as L
from tests import stream_order as SO

pytestmark = pytest.mark.gpu

SEQUENCES = ("default", "partial_batch", "fuse_layers=0", "fuse_pool_block=0", "input_gradient=0", "linear_wb_own_stream")
NETS = ("bn8", "bn32", "crcrl", "dropout", "ref")
CONTAINER_CASES = [f"{net}/{seq}" for net in NETS for seq in SEQUENCES if f"{net}/{seq}" in L.CASES]
# One gate per train step (see _LateBatch): a step's host-side enqueue is at most 0.5 ms (measured: profiles/stream_order.md), the
# harness's default gate is forty times that.
GATE_MS = SO.GATE_MS


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
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "host_layer_traces.json")))


class _LateBatch:
    """run_case's driver.  In front of EVERY train step of the sequence: the device is quiet, the batch and the labels hold a decoy, then
    the gate and the copies of the real ones are queued on S (and, gate_side, a gate on the thread's side stream).  A step is proven when
    the gates are still live once its calls have returned -- for the last one: once the flush behind it has returned.  That holds for
    the first step of a fresh net too, which sizes and allocates every layer (profiles/stream_order.md, "Found")."""

    def __init__(self, H, gate_side, gate_ms):
        self.H, self.gate_side, self.gate_ms = H, gate_side, gate_ms
        self.steps = []  # per train step: [live in front of it, live behind it, enqueue ms]

    def before_steps(self, xd, ld):
        T = self.H.T
        self.xd, self.ld = xd, ld
        self.real_x, self.real_l = xd.clone(), ld.clone()
        self.decoy_x = T.from_numpy(SO.decoy_of(self.real_x.cpu().numpy(), 7801)).cuda()
        self.decoy_l = (self.real_l + 1) % 3  # every label wrong
        self.H.keep.append(self)

    def before_op(self, i, op):
        if op[0] != "step":
            return
        H, T = self.H, self.H.T
        self._close()
        T.cuda.synchronize()
        self.xd.copy_(self.decoy_x)
        self.ld.copy_(self.decoy_l)
        T.cuda.synchronize()
        self.events = [H.gate(H.side, self.gate_ms)] if self.gate_side else []
        with T.cuda.stream(H.S):
            self.events.append(H.gate(H.S, self.gate_ms))
            self.xd.copy_(self.real_x, non_blocking=True)
            self.ld.copy_(self.real_l, non_blocking=True)
        self.steps.append([not any(ev.query() for ev in self.events), None, None])
        self.t0 = time.perf_counter()

    def after_op(self, i, op):
        pass

    def _close(self):
        if self.steps and self.steps[-1][1] is None:
            self.steps[-1][1:] = [not any(ev.query() for ev in self.events), (time.perf_counter() - self.t0) * 1e3]

    def after_steps(self):
        self._close()


@pytest.mark.parametrize("gate_side", [False, True], ids=["caller_late", "caller_late_side_gated"])
@pytest.mark.parametrize("name", CONTAINER_CASES)
def test_container_on_a_caller_stream(T, H, golden, lib_option, name, gate_side):
    """the sequence once ungated on S (first-call costs; its digests are the recorded ones as well), then gated: parameters, gradients,
    every layer's output, the input delta and the loss as recorded"""
    from cnn_amd import hostapi

    lib_option("IGEMM_AUTOTUNE", 0)  # (as the recorder: tile choice must not be a per-process measurement)
    lib = hostapi.load()
    lib.cnnh_set_stream(C.c_void_p(H.S.cuda_stream))
    try:
        plain = L.run_case(T, name)
        assert plain["sha"] == golden[name]["sha"], f"{name}: ungated on S"
        driver = _LateBatch(H, gate_side, GATE_MS)
        got = L.run_case(T, name, driver)
        H.enqueue_ms[f"container {name}{' side gated' if gate_side else ''}"] = [st[2] for st in driver.steps]
        assert all(st[0] and st[1] for st in driver.steps), f"{name}: a step's gate ended before the step was queued: {driver.steps}"
        assert got["sha"] == golden[name]["sha"], f"{name}: gated"
    finally:
        lib.cnnh_set_stream(None)
        T.cuda.synchronize()
