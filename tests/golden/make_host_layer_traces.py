#!/usr/bin/env python3
"""Records tests/golden/host_layer_traces.json: for every call sequence of tests/host_layer_cases.py the launch log
("<kernel>|<geometry>" -> launches) and a SHA-256 of the parameters, the gradients, every layer's output, the input delta where it is
valid and the loss, on seeded inputs with IGEMM_AUTOTUNE=0.  Needs the GPU and built libraries.

Every case runs twice on a fresh net; the script refuses to write the file when a record does not repeat.  The file was first recorded
with the host library of the commit before the layer classes were rebuilt from shared parts; a change that re-routes, re-fuses or
renames a kernel of these sequences on purpose re-records it with this script and says so.
usage: python tests/golden/make_host_layer_traces.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch

from cnn_amd import capi
from tests import host_layer_cases as L

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "host_layer_traces.json")
with capi.option("IGEMM_AUTOTUNE", 0):
    rec, unstable = L.trace_record(torch, repeats=2)
if unstable:
    sys.exit(f"records do not repeat, nothing written: {unstable}")
json.dump(rec, open(out, "w"), indent=0, sort_keys=True)
print(f"{len(rec)} cases -> {out}")
