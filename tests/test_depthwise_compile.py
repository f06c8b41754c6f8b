"""The depthwise layer at the public boundary, checked with a compiler and without a device: tests/caller/depthwise_caller.cpp -- a
Sequential with architectures::DepthwiseConv2D layers, the layer through the Layer virtuals, build_mobilenet_v1 and a
CNN_CONV2D_DEPTHWISE desc through the plain C entry points -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "depthwise_caller.cpp")


def test_depthwise_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
