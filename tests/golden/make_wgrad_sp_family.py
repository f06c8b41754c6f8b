#!/usr/bin/env python3
"""Records tests/golden/wgrad_sp_family.json: for every case of tests/wgrad_sp_cases.py (each instance and epilogue path of
conv_wgrad_sp.hip / conv_wgrad_sp2.hip / conv_wgrad_sp_any.hip, under the default stage partition and SP_BLOCKS = 1 and 3) the launch
log of one backward_weight call and a SHA-256 of gw and gb, on seeded inputs.  Needs the GPU and built libraries.

Every call runs twice.  These kernels sum in a fixed order: a digest that does not repeat is a finding, and the script refuses to
write the file.  The file was first recorded with the library of the commit before wgrad_sp_common.h existed (CNN_AMD_LIB=<path>
records from another build; <commit> is kept in the file); a change that renames, retunes or re-routes one of these kernels on purpose
re-records it with this script and says so.
usage: python tests/golden/make_wgrad_sp_family.py <commit the library was built from> [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch

from tests import wgrad_sp_cases as S

if len(sys.argv) < 2:
    sys.exit(__doc__)
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "wgrad_sp_family.json")
rec, unstable = S.family_record(torch, repeats=2)
for name in unstable:
    print("digest does not repeat:", name)
if unstable:
    sys.exit(f"{len(unstable)} calls do not repeat their digests: not recorded")
wrong = [w for w, r in rec.items() if not any(k.startswith(r["kernel"]) for k in r["log"])]
if wrong:
    sys.exit(f"not served by the kernel the case is meant for: {wrong}")
json.dump({"recorded_with": sys.argv[1], "records": rec}, open(out, "w"), indent=0, sort_keys=True)
print(f"{len(rec)} calls -> {out}")
