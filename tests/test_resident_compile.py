"""The device-resident dataset at the public boundary, checked with a compiler and without a device: tests/caller/resident_caller.cpp --
architectures::ResidentDataset and architectures::ResidentLoader (cnn_amd/host/include/resident.h) over cnn_dataset_* and
cnn_batch_stager_create_u8_resident / _indices / _labels of include/cnn_amd.h, one epoch of Sequential::train_step and one pass of
eval_step -- compiles against the public headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include")]
TU = os.path.join(ROOT, "tests", "caller", "resident_caller.cpp")


def test_resident_caller_compiles_against_the_public_headers():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", *INC, TU], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_resident_header_stands_alone_over_the_c_abi():
    """resident.h needs include/cnn_amd.h and nothing else of the project"""
    src = '#include "resident.h"\nint main() { return sizeof(architectures::ResidentLoader::Batch) > 0 ? 0 : 1; }\n'
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-x", "c++", *INC, "-"], input=src, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
