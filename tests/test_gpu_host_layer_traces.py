"""The C++ host layers (cnn_amd/host) against tests/golden/host_layer_traces.json -- which kernels every call sequence of
tests/host_layer_cases.py launches and the bytes it leaves behind, recorded by tests/golden/make_host_layer_traces.py with the host
library of the commit before the layer classes were rebuilt from shared parts -- and the two properties that rebuild makes sound: no
fusion mark outlives its pass, and Layer::get_output() returns what the last pass produced."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import host_layer_cases as L
from tests.util import uniform01

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "host_layer_traces.json")))


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(L.CASES)


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_host_layer_trace_matches_the_recorded_one(name, golden, lib_option):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    lib_option("IGEMM_AUTOTUNE", 0)  # (tile choice must not be a per-process measurement)
    got, want = L.run_case(torch, name), golden[name]
    assert got["log"] == want["log"]
    assert got["sha"] == want["sha"]


def _bn8(torch):
    net, names, layout, in_shape, B = L.build("bn8")
    x = uniform01(7700, (B,) + in_shape)
    labels = (np.arange(B) % 3).astype(np.int32)
    return net, names, layout, x, torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()


def test_a_backward_mark_does_not_outlive_its_pass(lib_option):
    """Sequential::grad_cam stops its backward walk at the ReLU between BatchNorm2D and the pool: the pool's backward has armed
    BatchNorm2D's "done by the pool" mark, BatchNorm2D::backward never ran to consume it.  With fuse_layers switched off the next
    pass' backward does not take the pooled path; the mark must not make BatchNorm2D::backward hand the delta through untouched.
    A twin net without the grad_cam call is the reference: gradients and parameters bit for bit."""
    import torch

    from cnn_amd import hostapi

    lib_option("IGEMM_AUTOTUNE", 0)
    lib = hostapi.load()
    got = []
    for with_cam in (True, False):
        net, names, layout, x, xd, ld = _bn8(torch)
        try:
            net.train_step(xd, ld, 1e-2)
            if with_cam:
                net.grad_cam("relu_layer_1", (xd.shape[0],) + tuple(layout[names.index("relu_layer_1")]["out"][1:]))
            lib.cnnh_set_fuse_layers(0)
            net.forward_backward(xd, ld)
            got.append((net.get_grads(), net.get_params()))
        finally:
            lib.cnnh_set_fuse_layers(1)
            net.close()
    assert np.array_equal(got[0][0], got[1][0]), float(np.abs(got[0][0] - got[1][0]).max())
    assert np.array_equal(got[0][1], got[1][1])


def test_get_output_returns_what_the_last_pass_produced(lib_option):
    """after a B = 2 train step, a forward pass of ONE sample: every layer's output is one sample (it fits a buffer of exactly that
    size) and equals what a fresh net makes of that sample bit for bit (the same one-sample pass: BatchNorm2D normalises over the batch
    it is given); grad_cam then returns a [1][H][W] map"""
    import torch

    lib_option("IGEMM_AUTOTUNE", 0)
    net, names, layout, x, xd, ld = _bn8(torch)
    fresh = L.build("bn8")[0]
    try:
        net.train_step(xd, ld, 0.0)  # (lr 0: the parameters stay the fresh net's; the moving statistics do not enter a training-mode forward)
        net.forward_host(x[:1])
        fresh.forward_host(x[:1])
        for lname, ent in zip(names, layout):
            one = np.empty((1,) + tuple(ent["out"]), np.float32)
            rc = net.lib.cnnh_net_layer_output(net.h, lname.encode(), one.ctypes.data_as(C.POINTER(C.c_float)), one.size)
            assert rc == 0, (lname, rc)
            want = fresh.layer_output(lname, (1,) + tuple(ent["out"]))
            assert np.array_equal(one[0], want[0]), lname
        H, W = layout[names.index("relu_layer_1")]["out"][1:]
        img, cam = net.grad_cam("relu_layer_1", (1, H, W))
        assert cam.shape == (1, H, W) and np.isfinite(cam).all()
    finally:
        net.close()
        fresh.close()
