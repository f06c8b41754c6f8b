"""The resident dataset's half-size levels at the public boundary, checked with a compiler and without a device:
tests/caller/mip_caller.cpp -- architectures::ResidentDataset with its `levels` argument, max_levels / levels / level_size / read_level
(cnn_amd/host/include/resident.h) and cnn_augment_level of include/cnn_amd.h -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "mip_caller.cpp")


def test_mip_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_the_levels_argument_defaults_to_one_level():
    """a caller written before the levels existed compiles unchanged, and the new argument is an int behind the three old ones"""
    src = ('#include "resident.h"\n'
           "int main() { architectures::ResidentDataset a(4, 8, 8); architectures::ResidentDataset b(4, 8, 8, 2);\n"
           "  return a.levels() + b.levels() + architectures::ResidentDataset::max_levels(8, 8); }\n")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-x", "c++", *INC, "-"], input=src, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
