"""Conv2D size queries and capability answers against tests/golden/conv_route_sizes.json (recorded by
tests/golden/make_conv_route_sizes.py with the library of the commit before the dispatch tables): needs no GPU."""
import json
import os

from tests import conv_route_cases as R


def test_conv_sizes_and_predicates_match_the_recorded_ones():
    """cnn_conv2d_workspace_bytes / _prepared_bytes / _relu_only_supported / _relu_maxpool2_supported / _pool_mask_packed_supported /
    _pool_mask_bytes of 150 descs, and of a dozen of them under WGRAD_RD=0, NO_DIRECT=1 and PK_DGRAD=1: every answer as recorded"""
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "conv_route_sizes.json")))
    assert golden["fields"] == R.SIZE_FIELDS
    got = R.size_record()
    assert sorted(got) == sorted(golden["answers"])
    assert len(got["default"]) >= 120 + 30 and all(len(got[f"{n}={v}"]) == 12 for n, v in R.OPTIONS)
    for variant, answers in golden["answers"].items():
        assert sorted(got[variant]) == sorted(answers), variant
        wrong = {k: (got[variant][k], v) for k, v in answers.items() if got[variant][k] != v}
        assert not wrong, (variant, wrong)
