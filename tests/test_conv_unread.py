"""tests/conv_unread.unread_mask against an enumeration of all windows, and the premise tests/test_gpu_operand_contract.py relies on:
the CPU oracle alone never lets a dead element of x into a result (conv2d.cpp:127-146) and writes +0.0 to its gradient (conv2d.cpp:168)."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import conv_route_cases as R
from tests.conv_unread import poisoned, unread_mask
from tests.util import normal_scaled, uniform01, uniform_pm1

WORDS = (0x7FC00000, 0x5A5A5A5A)  # the two poisons of tests/guarded.py


def _brute(case):
    H, W, k, s, pad = case[2], case[3], case[5], case[6], case[7]
    seen = np.zeros((H + 2 * pad, W + 2 * pad), bool)
    for oh in range((H + 2 * pad - k) // s + 1):
        for ow in range((W + 2 * pad - k) // s + 1):
            seen[oh * s:oh * s + k, ow * s:ow * s + k] = True
    return ~seen[pad:pad + H, pad:pad + W]


def test_unread_mask_is_the_enumeration_of_all_windows():
    cases = R.HAND_PICKED + R.sweep_cases()
    assert len(cases) == len(R.HAND_PICKED) + 120
    non_empty = 0
    for case in cases:
        m = unread_mask(case)
        assert m.dtype == bool and m.shape == (case[2], case[3]) and np.array_equal(m, _brute(case)), case
        non_empty += bool(m.any())
    assert non_empty >= 10  # (the first layer, the stride-3 desc, the 1x1 stride-2 lattice, ...: the GPU test has something to poison)


def test_unread_mask_of_the_descs_the_issue_names():
    m = unread_mask((2, 3, 224, 224, 16, 3, 2, 0))
    assert m[223].all() and m[:, 223].all() and not m[:223, :223].any()
    m = unread_mask((3, 32, 9, 11, 48, 1, 2, 0))  # 1x1 stride 2: only the even lattice is read
    assert not m[::2, ::2].any() and m[1::2].all() and m[:, 1::2].all()
    assert not unread_mask((2, 64, 56, 56, 128, 3, 2, 1)).any() and not unread_mask((2, 32, 7, 7, 64, 3, 1, 1)).any()
    assert unread_mask((1, 20, 17, 19, 130, 3, 3, 0))[15:].all()  # stride 3: rows 15, 16 lie behind the last window (12..14)


DEAD = [c for c in R.HAND_PICKED if unread_mask(c).any()]


@pytest.mark.parametrize("case", DEAD, ids=R.key)
def test_the_oracle_never_reads_a_dead_element(case):
    B, Ci, H, W, Co, k, s, pad = case[:8]
    mask = unread_mask(case)
    x, w, b = uniform01(31, (B, Ci, H, W)), normal_scaled(32, (Co, Ci, k, k)), normal_scaled(33, (Co,))
    dy = uniform_pm1(34, (B, Co, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1))

    def run(x_):
        xp = np.pad(x_, ((0, 0), (0, 0), (pad, pad), (pad, pad))) if pad else x_
        y = O.conv2d_forward(xp, w, b, s)
        gw, gb, dxp = O.conv2d_backward(xp, dy, w, s)
        return y, gw, gb, (dxp[:, :, pad:pad + H, pad:pad + W] if pad else dxp)

    x0 = x.copy()
    x0[:, :, mask] = 0
    want = run(x0)
    assert np.all(np.ascontiguousarray(want[3][:, :, mask]).view(np.uint32) == 0), "dx is +0.0 at the dead positions"
    assert np.any(want[3][:, :, ~mask] != 0)
    for word in WORDS:
        xq = poisoned(x, mask, word)
        assert np.all(xq.view(np.uint32)[:, :, mask] == word) and np.array_equal(xq[:, :, ~mask], x[:, :, ~mask])
        got = run(xq)
        for name, a, c in zip(("y", "gw", "gb", "dx"), got, want):
            assert a.shape == c.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(c).view(np.uint32)), (name, hex(word))
