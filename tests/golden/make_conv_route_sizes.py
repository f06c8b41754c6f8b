#!/usr/bin/env python3
"""Records tests/golden/conv_route_sizes.json: what the size queries and capability questions of the Conv2D entry points answer for
the fixed desc list of tests/conv_route_cases.py (the 120 random 3x3 geometries of the parity sweep, ~30 hand-picked descs, a dozen
of them again under WGRAD_RD=0 / NO_DIRECT=1 / PK_DGRAD=1).  Needs the built library, no GPU (without a device the planners size
their grids for 256 compute units, the MI355X's own count).

The file was first recorded with the library of the commit before the dispatch tables existed; a change that moves a size or an
answer on purpose re-records it with this script and says so.  CNN_AMD_LIB=<path> records from another build of the library.
usage: python tests/golden/make_conv_route_sizes.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import conv_route_cases as R

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_route_sizes.json")
rec = R.size_record()
json.dump({"fields": R.SIZE_FIELDS, "answers": rec}, open(out, "w"), indent=0, sort_keys=True)
print(f"{sum(len(v) for v in rec.values())} descs -> {out}")
