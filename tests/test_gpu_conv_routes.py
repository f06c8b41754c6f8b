"""Which kernels every Conv2D call launches, and the bytes it writes, against tests/golden/conv_routes.json (recorded by
tests/golden/make_conv_routes.py with the library of the commit before the dispatch tables)."""
import json
import os

import pytest

from tests import conv_route_cases as R

pytestmark = pytest.mark.gpu


def test_conv_routes_and_results_match_the_recorded_ones():
    """~30 hand-picked descs x (forward, forward + ReLU, data gradient, data gradient + ReLU', weight gradient, the prepared variants
    behind one prepare_filters call per six layers, forward / data gradient without a workspace and with one offset by 4 bytes): the
    launch log of every call and the SHA-256 of every output as recorded (a call recorded without digests compares its log only)"""
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "conv_routes.json")))
    got, _ = R.route_record(torch)
    assert sorted(got) == sorted(golden)
    wrong = {}
    for where, calls in golden.items():
        assert sorted(got[where]) == sorted(calls), where
        for name, want in calls.items():
            have = got[where][name] if "sha" in want or "rc" in want else {"log": got[where][name]["log"]}
            if have != want:
                wrong[f"{where}:{name}"] = (have, want)
    assert not wrong, wrong
