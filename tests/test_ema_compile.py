"""The parameter average at the public boundary, checked with a compiler and without a device: tests/caller/ema_caller.cpp -- the new
Sequential members (set_ema, reset_ema, swap_ema, ema_swapped, ema_device, ema_decay, ema_updates, ema_active, save_ema_state,
load_ema_state) and cnn_ema_decay_at / cnn_ema_update / cnn_arena_swap of include/cnn_amd.h -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "ema_caller.cpp")


def test_ema_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
