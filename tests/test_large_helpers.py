"""The helpers of the large-tensor tests (tests/large.py), without a device: the batch sizes at the documented limits (DESIGN.md section
11) and the restatement of the magic division that the pooled-domain BatchNorm regression plants its inputs with."""
import numpy as np
import pytest

from tests.large import batch_under, misdecoded_rows, misdecoded_slot_starts


@pytest.mark.parametrize("per,limit,under", [(64 * 112 * 112, 1 << 29, 668), (128 * 28 * 28, 1 << 29, 5349), (64 * 56 * 56, 1 << 29, 2674),
                                             (16 * 111 * 111, 1 << 29, 2723), (16 * 111 * 111, ((1 << 31) - 16) // 4, 2723),
                                             (3 * 224 * 224, ((1 << 31) - 16) // 4, 3566), (16 * 111 * 111, 1 << 31, 10893),
                                             (128 * 112 * 112, 1 << 31, 1337), (64 * 112 * 112, 1 << 31, 2674), (64 * 112 * 112, 1 << 32, 5349)])
def test_batch_under_is_the_last_batch_below_the_limit(per, limit, under):
    B = batch_under(per, limit)
    assert B == under and B * per < limit <= (B + 1) * per


def test_batch_under_at_an_exact_multiple():
    assert batch_under(4, 16) == 3 and batch_under(4, 17) == 4


@pytest.mark.parametrize("plane,count", [((112, 112), 0), ((140, 120), 0), ((74, 76), 0), ((1720, 1720), 255), ((130, 5956), 1), ((2044, 2044), 1000),
                                         ((12, 39780), 23), ((16, 36604), 34)])
def test_uncorrected_magic_division_restated(plane, count):
    H, W = plane
    bad = misdecoded_rows(H, W)
    assert len(bad) == count
    # the quotient is one too high there and nowhere else: one correction step makes the division exact on the whole plane
    magic = ((1 << 32) + W - 1) // W
    hw = np.arange(H * W, dtype=np.uint64)
    h = (hw * np.uint64(magic)) >> np.uint64(32)
    assert np.array_equal(np.nonzero(h == hw // np.uint64(W) + np.uint64(1))[0], bad)
    h = h - (h * np.uint64(W) > hw)
    assert np.array_equal(h, hw // np.uint64(W))


@pytest.mark.parametrize("plane,starts", [((112, 112), []), ((1720, 1720), []), ((130, 5956), []), ((2044, 2044), []), ((12, 39780), [437576]),
                                          ((16, 36604), [475848, 549056])])
def test_slot_starts_the_pooled_batchnorm_kernels_would_misdecode(plane, starts):
    """what the regression in tests/test_gpu_batchnorm.py rests on: only the last two planes have a mis-decoded element that is the first
    of an aligned 4-element slot in an even row (the one the kernels decode, at the parity where the window changes)"""
    H, W = plane
    got = misdecoded_slot_starts(H, W)
    assert got.tolist() == starts
    assert all(hw % 4 == 0 and (hw // W) % 2 == 0 and hw % W == W - 4 for hw in got)
