"""The photometric half at the public boundary, checked with a compiler and without a device: tests/caller/photo_caller.cpp --
architectures::PhotoAugmentor (cnn_amd/host/include/augment.h), the photo stager (cnn_batch_stager_create_u8_photo / _photo /
_set_normalize) and cnn_colour_matrix of include/cnn_amd.h -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "photo_caller.cpp")


def test_photo_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
