"""What a batch stager's slot holds (cnn_amd/csrc/stager_layout.h: StagerKind, stager_has, slot_layout), held to the layout that
include/cnn_amd.h documents by tests/caller/stager_layout_check.cpp under AddressSanitizer and UBSan -- a stand-alone program on the CPU:
no device, no libcnn_amd.so, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_stager_layout_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stager_layout_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
           "-I" + os.path.join(ROOT, "cnn_amd", "csrc"), os.path.join(ROOT, "tests", "caller", "stager_layout_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "warning" not in out.stderr, out.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout[-3000:], run.stderr[-3000:])
