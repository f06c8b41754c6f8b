"""Device-side augmentation at the public boundary, checked with a compiler and without a device: tests/caller/augment_caller.cpp --
architectures::ImageAugmentor (cnn_amd/host/include/augment.h), the augmenting stager (cnn_batch_stager_create_u8_aug / _matrices /
_set_fill) and cnn_augment_matrix / cnn_augment_u8 of include/cnn_amd.h -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "augment_caller.cpp")


def test_augment_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
