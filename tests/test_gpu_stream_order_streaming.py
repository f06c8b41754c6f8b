"""Stream order of the streaming entry points of elementwise.hip (tests/stream_order.py is the harness): every case of
tests/streaming_cases.py::case_list(SMALL) through its _call, caller late, against the digests of tests/golden/streaming.json."""
import json
import os

import pytest

from tests import stream_order as SO
from tests import streaming_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture
def H(T):
    h = SO.harness(T)
    try:
        yield h
    finally:
        h.finish()


def blocks_the_host(case):
    """by contract of the capi wrapper: clip_grad_norm waits for its workspace's lifetime, a range table beyond the inline limit is
    uploaded (a pageable copy) and kept alive by a wait"""
    entry, _, t, n, _ = case
    return entry.startswith("clip") or (t is not None and len(C.table(t, n)) > 64)


@pytest.mark.parametrize("n", C.SMALL)
def test_streaming_cases_caller_late(T, H, n):
    """the four seeded arrays of one size (and the second moment derived from them) arrive late on S; the case's own buffers are
    copied from them inside the call, behind the gate: the recorded bytes of every buffer the call may write"""
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "streaming.json")))["records"]
    I = C._Inputs(T, n)
    T.cuda.synchronize()
    late = [H.late(d, 7600 + 10 * (n % 100) + k) for k, d in enumerate(I.dev[:4])]
    late.append(H.late(I.dev[4], 0, decoy=late[3][2] * late[3][2]))  # (a second moment: not negative, in the decoy as well)
    cases = C.case_list([n])
    assert any(blocks_the_host(c) for c in cases) and not all(blocks_the_host(c) for c in cases)
    for case in cases:
        where = C.where(case)
        res = H.caller_late("streaming " + where, late, C._call(T, I, case), blocks=blocks_the_host(case))
        got = {name: SO.sha(a) for name, a in sorted(res.gated.items())}
        assert got == golden[where]["sha"], f"{where}: the gated call's bytes are not the recorded ones"
        res.assert_same_bits_as_plain(where)
