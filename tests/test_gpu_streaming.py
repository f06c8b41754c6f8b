"""Every entry point of elementwise.hip with the streaming shape against tests/golden/streaming.json (recorded by
tests/golden/make_streaming.py with the library of the commit before stream_walk existed)."""
import json
import os

import pytest

from tests import streaming_cases as S

pytestmark = pytest.mark.gpu


def test_case_list_is_what_it_claims():
    """(needs no device) every entry at every size and both alignments; every table at 1027; no table that cannot be formed"""
    sizes = S.SMALL + [S.past_a_full_grid(256)]
    assert sizes[-1] == 2098355
    cases = S.case_list(sizes)
    assert len({S.where(c) for c in cases}) == len(cases)
    for n in sizes:
        for off in (0, 1):
            here = [c for c in cases if c[3] == n and c[4] == off]
            assert {c[0] for c in here} == set(S.SIMPLE) | {"sgdm", "adam", "ema"}, (n, off)
            assert all(c[2] is None or S.table(c[2], n) is not None for c in here)
            for entry in ("sgdm", "adam", "ema"):
                have = {c[2] for c in here if c[0] == entry}
                assert have >= ({"none"} if n == 1 else {"none", "cut"} if n < 1027 else {"none", "cut", "many"}), (entry, n, have)
    assert len(S.table("many", 1027)) == S.MANY and all(len(S.table("cut", n)) == 3 for n in sizes[-2:])


def test_streaming_launches_and_bits_match_the_recorded_ones():
    """one call per case: the launch log and the SHA-256 of every buffer the call may write, as recorded; one record per case"""
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "streaming.json")))
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert cus == golden["compute_units"], "the largest size follows the compute-unit count: recorded on another device"
    golden = golden["records"]
    got, _ = S.streaming_record(torch)
    assert sorted(got) == sorted(golden)
    assert len(golden) == len(S.case_list(S.sizes_of(torch)))
    wrong = {}
    for where, want in golden.items():
        assert want["log"] and want["sha"], where
        if got[where] != want:
            wrong[where] = (got[where], want)
    assert not wrong, dict(list(wrong.items())[:10])
