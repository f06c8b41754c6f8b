"""The soft-target steps at the public boundary, checked with a compiler and without a device: tests/caller/soft_targets_caller.cpp --
Sequential::set_label_smoothing, train_step_mixed, train_step_soft, last_targets_device and cnn_batch_mix / cnn_soft_targets /
cnn_cutmix_lambda / cnn_softmax_xent_soft of include/cnn_amd.h -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "soft_targets_caller.cpp")


def test_soft_targets_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
