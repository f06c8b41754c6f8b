"""The parts the host layers are made of (cnn_amd/host/include/layer_parts.h, src/layer_parts.cpp: Mark, Workspace, ParamBlock, write_back_staged), exercised by
tests/caller/layer_parts_check.cpp against stub cnn_* functions under AddressSanitizer and UBSan -- a stand-alone program on the CPU: no
device, no libcnn_amd.so."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_layer_parts_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "layer_parts_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-I" + os.path.join(ROOT, "cnn_amd", "host", "include"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "caller", "layer_parts_check.cpp"), os.path.join(ROOT, "cnn_amd", "host", "src", "layer_parts.cpp"),
           os.path.join(ROOT, "cnn_amd", "host", "src", "tensor3d.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    run = subprocess.run([exe, str(tmp_path / "block.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-3000:])
