"""Device-side evaluation at the public boundary, checked with a compiler and without a device: tests/caller/eval_caller.cpp -- the new
Sequential members (eval_begin, eval_step, eval_result, last_predictions_device), architectures::EvalResult and cnn_eval_state_bytes /
cnn_eval_accumulate / cnn_eval_read of include/cnn_amd.h -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "eval_caller.cpp")


def test_eval_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
