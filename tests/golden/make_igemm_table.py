#!/usr/bin/env python3
"""Records tests/golden/igemm_table.json: for every row of kTiles (cnn_amd/csrc/conv_igemm.hip), forced with CNN_AMD_IGEMM_CFG=<id>, the
launch log and a SHA-256 of the output of one forward and one data-gradient call on each desc of tests/igemm_table_cases.py, on the
lattice operands of tests/exact.py.  Needs the GPU and built libraries.

Every call runs twice.  These kernels sum in a fixed order: a digest that does not repeat is a finding, and the script refuses to
write the file.  It also refuses when a tile without a split rule launched its own kernel in none of its calls, and when a result is
not the integer truth.  The file was first recorded with the library of the commit before kTiles existed (CNN_AMD_LIB=<path> records
from another build; <commit> is kept in the file); a change that adds, renames or re-routes a tile on purpose re-records it with this
script and says so.
usage: python tests/golden/make_igemm_table.py <commit the library was built from> [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch

from tests import igemm_table_cases as S

if len(sys.argv) < 2:
    sys.exit(__doc__)
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "igemm_table.json")
rec, unstable, wrong = S.table_record(torch, repeats=2)
for name in unstable:
    print("digest does not repeat:", name)
if unstable:
    sys.exit(f"{len(unstable)} calls do not repeat their digests: not recorded")
for report in wrong:
    print(report)
if wrong:
    sys.exit(f"{len(wrong)} results are not the integer truth: not recorded")
idle = S.never_ran(rec)
if idle:
    sys.exit(f"tiles whose own kernel is in none of their launch logs: {idle}: not recorded")
refused = sorted(f"{where}:{call}" for where, calls in rec.items() for call, r in calls.items() if "rc" in r)
print(f"{len(refused)} calls refused (recorded with their code):", refused)
json.dump({"recorded_with": sys.argv[1], "records": rec}, open(out, "w"), indent=0, sort_keys=True)
print(f"{sum(len(c) for c in rec.values())} calls -> {out}")
