#!/usr/bin/env python3
"""Records tests/golden/conv_routes.json: for every hand-picked desc of tests/conv_route_cases.py and every Conv2D call (forward,
forward + ReLU, data gradient, data gradient + ReLU', weight gradient, the *_prepared variants behind one cnn_conv2d_prepare_filters
call per six layers, forward / data gradient with the workspace withheld and offset by 4 bytes) the launch log
("<kernel>|<geometry>" -> launches) and a SHA-256 of each output's bytes, on seeded inputs.  Needs the GPU and built libraries.

Every call runs twice; a call whose digests do not repeat keeps its launch log only and is printed -- more than two of them is a
finding, and the script refuses to write the file.  The file was first recorded with the library of the commit before the dispatch
tables existed (CNN_AMD_LIB=<path> records from another build); a change that renames, retunes or re-routes a kernel on purpose
re-records it with this script and says so.
usage: python tests/golden/make_conv_routes.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch

from tests import conv_route_cases as R

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_routes.json")
rec, unstable = R.route_record(torch, repeats=2)
for name in unstable:
    print("digest does not repeat, launch log only:", name)
if len(unstable) > 2:
    sys.exit(f"{len(unstable)} calls do not repeat their digests: not recorded")
json.dump(rec, open(out, "w"), indent=0, sort_keys=True)
print(f"{sum(len(v) for v in rec.values())} calls of {len(rec)} descs -> {out}")
