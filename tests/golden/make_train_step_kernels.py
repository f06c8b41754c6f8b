#!/usr/bin/env python3
"""Records tests/golden/train_step_kernels_before_optimizer.json: the launch log ("<kernel>|<geometry>" -> launches) of three
train_steps of the reference net at B = 16 with NO optimizer set, on the inputs of
tests/test_gpu_optimizer.py::test_default_path_is_untouched.  Needs the GPU and built libraries.

The file was first recorded with the libraries of the commit before the optimizer existed.  It pins the default path's kernels, so a
later change that renames, retunes or re-fuses a kernel of the reference net's step on purpose -- nothing to do with the optimizer --
must re-record it: run this script from the repository root on that change's build and commit the new file with it.
usage: python tests/golden/make_train_step_kernels.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from cnn_amd import capi, hostapi, stacks as S
from util import uniform01

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "train_step_kernels_before_optimizer.json")
p0 = S.he_init(S.walk(S.alexnet(3)), 340)
x = torch.from_numpy(uniform01(341, (16, 3, 224, 224))).cuda()
labels = torch.from_numpy((np.arange(16) % 3).astype(np.int32)).cuda()
net = hostapi.HostAlexNet(3)
net.set_params(p0)
torch.cuda.synchronize()
capi.kernel_timing(1)
for _ in range(3):
    net.train_step(x, labels, 1e-3)
net.flush()
rep = capi.kernel_timing_report()
capi.kernel_timing(0)
net.close()
json.dump({k: cnt for k, (cnt, _) in rep.items()}, open(out, "w"), indent=1, sort_keys=True)
print(f"{len(rep)} keys -> {out}")
