"""Every row of kTiles (cnn_amd/csrc/conv_igemm.hip) against tests/golden/igemm_table.json (recorded by tests/golden/make_igemm_table.py
with the library of the commit before the table existed) and against the integer truth of tests/exact.py."""
import json
import os

import pytest

from tests import igemm_table_cases as S
from tests import igemm_tiles as G

pytestmark = pytest.mark.gpu


def test_every_tile_launches_and_computes_what_was_recorded():
    """every id of the table forced through IGEMM_CFG, one forward and one data-gradient call on each of the three descs: the launch
    log and the SHA-256 of the output as recorded (a refusal: its code), every result the integer truth bit for bit -- the digests alone
    would pass a bug the recording library had -- and every tile without a split rule with its own kernel in at least one log"""
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "igemm_table.json")))["records"]
    try:
        got, _, wrong = S.table_record(torch)
    except S.DeviceError as e:
        pytest.exit(f"device error in tests/test_gpu_igemm_table.py: {e}", returncode=3)
    assert sorted(got) == sorted(golden)
    assert len(golden) == len(G.source_table()) * len(S.DESCS)
    assert not wrong, wrong
    differ = {}
    for where, want in golden.items():
        assert sorted(want) == sorted(S.CALLS), where
        for call, r in want.items():
            assert ("sha" in r) != ("rc" in r), (where, call)
        if got[where] != want:
            differ[where] = (got[where], want)
    assert not differ, differ
    assert S.never_ran(got) == []
