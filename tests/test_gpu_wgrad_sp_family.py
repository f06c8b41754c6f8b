"""Every instance and epilogue path of the LDS-staged output-stationary weight gradients against tests/golden/wgrad_sp_family.json
(recorded by tests/golden/make_wgrad_sp_family.py with the library of the commit before wgrad_sp_common.h existed)."""
import json
import os

import pytest

from tests import wgrad_sp_cases as S

pytestmark = pytest.mark.gpu


def test_wgrad_sp_family_launches_and_bits_match_the_recorded_ones():
    """17 descs (25 with the 4-byte DMA instances) x (default partition, SP_BLOCKS = 1, SP_BLOCKS = 3), one backward_weight call each:
    the launch log and the SHA-256 of gw and gb as recorded -- no record without digests: these kernels sum in a fixed order -- and
    the kernel the case is meant for in the log (a case silently served by another family would otherwise pass)"""
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "wgrad_sp_family.json")))["records"]
    got, _ = S.family_record(torch)
    assert sorted(got) == sorted(golden)
    assert len(golden) == 3 * (2 * len(S.SP) + len(S.SP2) + len(S.SPA))
    wrong = {}
    for where, want in golden.items():
        assert sorted(want["sha"]) == ["gb", "gw"], where
        have = got[where]
        assert any(k.startswith(have["kernel"]) for k in have["log"]), (where, have["log"])
        if have != want:
            wrong[where] = (have, want)
    assert not wrong, wrong
