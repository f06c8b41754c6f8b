"""The two host halves of the resident dataset's half-size levels (include/cnn_amd.h: cnn_augment_level, cnn_dataset_max_levels) against
their restatement in tests/mip_ref.py, bit for bit, and the restatement's own premises.  No device needed."""
import ctypes as C

import numpy as np
import pytest

from tests import mip_ref as M

F = np.float32


def same(m, L):
    """cnn_augment_level and mip_ref.choose on the same map -> (level, map); asserts they agree to the bit"""
    from cnn_amd import capi

    m = np.asarray(m, dtype=F)
    got_l, got_m = capi.augment_level(m, L)
    want_l, want_m = M.choose(m, L)
    assert got_l == want_l, (m, L, got_l, want_l)
    assert got_m.tobytes() == want_m.tobytes(), (m, L, got_m, want_m)
    return got_l, got_m


def test_plain_resize_maps():
    from cnn_amd import capi

    l, m = same(capi.augment_matrix([], 64, 64, 16, 16), 3)  # shrink 4: level 2 is 16 x 16, the map on it the identity exactly
    assert l == 2 and m.tobytes() == np.array([1, 0, 0, 0, 1, 0], F).tobytes()
    l, m = same(capi.augment_matrix([], 64, 64, 33, 33), 3)  # shrink 64 / 33 < 2
    assert l == 0 and m.tobytes() == capi.augment_matrix([], 64, 64, 33, 33).tobytes()
    l, m = same(capi.augment_matrix([], 64, 64, 32, 32), 3)  # r == 2.0: the boundary belongs to the level above
    assert l == 1 and m.tobytes() == np.array([1, 0, 0, 0, 1, 0], F).tobytes()
    l, _ = same(capi.augment_matrix([], 64, 48, 16, 24), 4)  # rx = 2, ry = 4: the larger one decides
    assert l == 2


def test_rotations_and_flips():
    from cnn_amd import capi

    rot = capi.augment_matrix([(capi.AUG_ROTATE, 30.0)], 96, 96, 32, 32)
    l, m = same(rot, 4)
    assert l == 1  # r is 3 up to rounding: [2, 4)
    assert np.array_equal(m[[0, 1, 3, 4]], rot[[0, 1, 3, 4]] / F(2))  # (a division by a power of two is exact)
    for ops in ([(capi.AUG_HFLIP,)], [(capi.AUG_VFLIP,)], [(capi.AUG_HFLIP,), (capi.AUG_ROTATE, 30.0)]):
        l, m = same(capi.augment_matrix(ops, 96, 96, 32, 32), 4)
        assert l == 1
    flip = capi.augment_matrix([(capi.AUG_HFLIP,)], 96, 96, 32, 32)
    l, m = same(flip, 4)
    # the level-1 image is 48 wide: its mirrored resize to 32 is what the level map must be
    assert m.tobytes() == capi.augment_matrix([(capi.AUG_HFLIP,)], 48, 48, 32, 32).tobytes()
    rs = np.random.RandomState(5)
    for _ in range(200):
        same(rs.standard_normal(6).astype(F) * F(rs.choice([0.5, 2, 7, 40])), int(rs.randint(1, 15)))


def test_one_level_is_always_level_0():
    from cnn_amd import capi

    for m in (capi.augment_matrix([], 64, 64, 4, 4), np.array([100, 0, 3, 0, 100, 5], F), np.array([1, 0, 0, 0, 1, 0], F)):
        l, out = same(m, 1)
        assert l == 0 and out.tobytes() == np.asarray(m, F).tobytes()


def test_demand_above_the_last_level_is_clamped():
    from cnn_amd import capi

    m = capi.augment_matrix([], 64, 64, 2, 2)  # shrink 32: level 5 of a long enough chain
    assert same(m, 14)[0] == 5
    l, out = same(m, 3)
    assert l == 2 and out[0] == F(8) and out[4] == F(8)  # the residual ratio is then above 2


def test_non_finite_entries_give_level_0():
    for k in (0, 1, 3, 4):
        for bad in (np.nan, np.inf, -np.inf):
            m = np.array([8, 0, 1, 0, 8, 1], F)
            m[k] = bad
            l, out = same(m, 4)
            assert l == 0 and out.tobytes() == m.tobytes()
    m = np.array([np.inf, np.nan, 1, np.nan, np.inf, 1], F)
    assert same(m, 4)[0] == 0
    big = np.array([3e38, 0, 0, 0, 3e38, 0], F)  # finite in fp32, and its square is finite in double
    assert same(big, 4)[0] == 3


def test_level_0_keeps_the_map_bit_for_bit():
    m = np.array([1.5, 0, 1e-20, 0, 1.5, -1e-20], F)  # (m2 + 0.5) - 0.5 would lose m2
    l, out = same(m, 4)
    assert l == 0 and out.tobytes() == m.tobytes() and out[2] == F(1e-20)
    neg = np.array([-0.0, 1, 0, 1, -0.0, 0], F)  # a quarter turn with its negative zeros
    l, out = same(neg, 4)
    assert l == 0 and out.tobytes() == neg.tobytes()


def test_refusals():
    from cnn_amd import capi

    lib = capi.load()
    m = (C.c_float * 6)(1, 0, 0, 0, 1, 0)
    out, level = (C.c_float * 6)(), C.c_int()
    assert lib.cnn_augment_level(m, 0, C.byref(level), out) == 1 and b"levels" in lib.cnn_amd_last_error()
    assert lib.cnn_augment_level(m, 15, C.byref(level), out) == 1
    assert lib.cnn_augment_level(None, 2, C.byref(level), out) == 1 and b"null" in lib.cnn_amd_last_error()
    assert lib.cnn_augment_level(m, 2, None, out) == 1 and lib.cnn_augment_level(m, 2, C.byref(level), None) == 1
    assert lib.cnn_augment_level(m, 2, C.byref(level), m) == 0  # in place


def test_max_levels():
    from cnn_amd import capi

    assert capi.dataset_max_levels(1, 1) == 1
    assert capi.dataset_max_levels(5, 7) == 4
    assert capi.dataset_max_levels(8192, 3) == 14
    for hs, ws in ((1, 1), (5, 7), (8192, 3), (3, 5), (2, 2), (33, 17), (1, 9), (1024, 1024)):
        assert capi.dataset_max_levels(hs, ws) == M.max_levels(hs, ws)
    lib = capi.load()
    for hs, ws in ((0, 4), (4, 0), (-1, 4), (4, -3), (8193, 1)):
        assert lib.cnn_dataset_max_levels(hs, ws) == 0 and b"cnn_dataset_max_levels" in lib.cnn_amd_last_error()
        with pytest.raises(capi.CnnAmdError):
            capi.dataset_max_levels(hs, ws)


def test_halve_by_hand():
    """the restatement's own premises: the rule on values worked out by hand"""
    img = np.zeros((3, 5, 3), np.uint8)
    img[..., 0] = [[0, 1, 2, 3, 4], [10, 11, 12, 13, 14], [20, 21, 22, 23, 24]]
    img[..., 1] = 255
    img[..., 2] = [[1, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 1, 0, 1]]
    got = M.halve(img)
    assert got.shape == (2, 3, 3)
    # (0+1+10+11+2)>>2 = 6, (2+3+12+13+2)>>2 = 8, the last column replicated: (4+4+14+14+2)>>2 = 9; the last row replicated as well
    assert got[..., 0].tolist() == [[6, 8, 9], [21, 23, 24]]
    assert (got[..., 1] == 255).all()
    # 1/4 rounds down ((1 + 2) >> 2 = 0), 2/4 rounds up ((1 + 0 + 1 + 0 + 2) >> 2 = 1 in the replicated last row), 4/4 is 1
    assert got[..., 2].tolist() == [[0, 0, 0], [0, 1, 1]]
    levels = M.chain(img, 3)
    assert [lv.shape[:2] for lv in levels] == [(3, 5), (2, 3), (1, 2)]
    col = np.tile(np.array([0, 255, 255, 0], np.uint8), 16)
    stripes = np.broadcast_to(col[None, :, None], (64, 64, 3)).copy()
    assert (M.chain(stripes, 3)[2] == 128).all()  # (0 + 255 + 0 + 255 + 2) >> 2 = 128, then (4 * 128 + 2) >> 2 = 128
