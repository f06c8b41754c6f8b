#!/usr/bin/env python3
"""Records tests/golden/streaming.json: for every case of tests/streaming_cases.py (each entry point of elementwise.hip with the
streaming shape, at the sizes, alignments and range tables listed there) the launch log of one call and a SHA-256 of every buffer the
call may write, on seeded inputs.  Needs the GPU and the built library.

Every call runs twice.  These kernels sum in a fixed order or not at all: a digest that does not repeat is a finding, and the script
refuses to write the file.  The largest size follows the device's compute-unit count, which the file keeps.  The file was first
recorded with the library of the commit before stream_walk existed (CNN_AMD_LIB=<path> records from another build; <commit> is kept in
the file); a change that renames or re-routes one of these kernels on purpose re-records it with this script and says so.
usage: python tests/golden/make_streaming.py <commit the library was built from> [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch

from tests import streaming_cases as S

if len(sys.argv) < 2:
    sys.exit(__doc__)
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "streaming.json")
rec, unstable = S.streaming_record(torch, repeats=2)
for name in unstable:
    print("digest does not repeat:", name)
if unstable:
    sys.exit(f"{len(unstable)} calls do not repeat their digests: not recorded")
cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
json.dump({"recorded_with": sys.argv[1], "compute_units": cus, "records": rec}, open(out, "w"), indent=0, sort_keys=True)
print(f"{len(rec)} calls -> {out}")
