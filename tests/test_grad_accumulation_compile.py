"""Gradient accumulation at the public boundary, checked with a compiler and without a device: tests/caller/grad_accumulation_caller.cpp
-- the four new Sequential members (set_grad_accumulation, grad_accumulation, accumulation_phase, accumulated_grads_device) and
cnn_grad_accumulate of include/cnn_amd.h -- compiles against the public headers; the library exports the entry and refuses bad
arguments before it touches a device; the handle API exports its three entries."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "grad_accumulation_caller.cpp")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@needs_gxx
def test_grad_accumulation_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Wno-unused-parameter", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_entry_is_exported_and_bound():
    from cnn_amd import capi, hostapi

    lib = capi.load()
    assert hasattr(lib, "cnn_grad_accumulate")
    assert capi.SIGNATURES["cnn_grad_accumulate"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p])
    assert lib.cnn_amd_abi_version() == 2
    syms = subprocess.run(["nm", "-D", "--defined-only", hostapi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("cnnh_net_set_grad_accumulation", "cnnh_net_accumulation_phase", "cnnh_net_get_accumulated_grads"):
        assert f" T {name}\n" in syms and name in hostapi.SIGNATURES, name


def test_refusals_come_before_any_launch():
    """null pointers, n == 0 and acc == grads: CNN_AMD_E_BADARG with a message naming the entry -- on a machine without a device, so
    nothing was launched"""
    from cnn_amd import capi

    lib = capi.load()
    a, b = (C.c_float * 8)(), (C.c_float * 8)()  # (host memory: the checks never dereference)
    pa, pb = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p)
    for args, word in (((None, pb, 8, 1, None), b"null"), ((pa, None, 8, 0, None), b"null"), ((pa, pb, 0, 1, None), b"n=0"),
                       ((pa, pa, 8, 0, None), b"same buffer")):
        assert lib.cnn_grad_accumulate(*args) == 1, args
        msg = lib.cnn_amd_last_error()
        assert msg.startswith(b"cnn_grad_accumulate") and word in msg, msg
