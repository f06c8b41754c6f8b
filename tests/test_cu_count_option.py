"""The CUS switch on the host side: num_cus() answers min(CUS, the device's compute units) for CUS >= 1, the
device's own count otherwise -- seen here through the size queries, which need no device (num_cus() then falls back to 256).

Three descs whose workspace is a slab family's and so a function of the CU count (a workspace holds the slabs, one more slab row per
64 of them for the reduction's first stage, and 64 floats of slack):
  STEM (4, 3, 64, 64, 64, 7, 2, 3): conv_stem.hip's weight gradient writes gx = min(2 * cus / co_blocks, items) slabs of Co x 148 floats;
       co_blocks = 1, items = B * Ho * col_blocks = 4 * 32 * 1 = 128.  cus = 20 -> 40 slabs, 40 -> 80, >= 64 -> 128.  Below about 7 CUs
       another family's scratch (2048 * Co floats) is the larger one, so the small counts are read from C11B.
  C11B (8, 128, 28, 28, 128, 1, 1, 0): conv_1x1.hip's weight gradient writes min((2 * cus + blocks - 1) / blocks, pixels / 128) slabs of
       Co x (Ci + 1) floats; blocks = 1 row block of 128 x 1 ci block, pixels = 8 * 784 = 6272 (at most 49 slabs): 2 * cus slabs up to
       cus = 24, and the family's scratch is the desc's largest at every such count: cus = 1 -> 2 slabs, 2 -> 4, 5 -> 10, 7 -> 14.
  C11  (8, 64, 28, 28, 64, 1, 1, 0): the same family with Co = Ci = 64: 49 slabs (the pixel bound) from 25 CUs on."""
import ctypes as C
import os
import subprocess
import sys

from cnn_amd import capi
from tests import conv_route_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM = (4, 3, 64, 64, 64, 7, 2, 3)
C11B = (8, 128, 28, 28, 128, 1, 1, 0)
C11 = (8, 64, 28, 28, 64, 1, 1, 0)


def _ws(case):
    d = R.desc(case)
    return int(capi.load().cnn_conv2d_workspace_bytes(C.byref(d)))


def _sizes(case):
    d = R.desc(case)
    lib = capi.load()
    return int(lib.cnn_conv2d_workspace_bytes(C.byref(d))), int(lib.cnn_conv2d_prepared_bytes(C.byref(d)))


def _stem_bytes(slabs):
    return ((slabs + (slabs + 63) // 64) * 64 * 148 + 64) * 4


def _c11b_bytes(slabs):
    return ((slabs + (slabs + 63) // 64) * 128 * 129 + 64) * 4


def test_cus_is_parsed_and_clamped(lib_option):
    lib_option("CUS", None)
    own = _ws(STEM)
    # the device's own count as the stem sees it: min(2 * cus, 128) slabs -- 128 from 64 compute units on (256 without a device), fewer on
    # a smaller partition; the expectations below hold for either
    own_slabs = [n for n in range(1, 129) if _stem_bytes(n) == own]
    assert len(own_slabs) == 1, own
    for value in ("0", "-3", "100000"):  # not positive: the device's own count; above it: clamped to it
        lib_option("CUS", value)
        assert _ws(STEM) == own, value
    for n in (20, 40):
        lib_option("CUS", str(n))
        assert _ws(STEM) == _stem_bytes(min(2 * n, own_slabs[0])), n
    lib_option("CUS", "CNN")  # (atoll: no number reads as 0)
    assert _ws(STEM) == own
    for n in (1, 2, 5, 7):  # the small counts, to the slab: a clamp that made 1 into 2 or 5 into 7 shows
        lib_option("CUS", str(n))
        assert _ws(C11B) == _c11b_bytes(2 * n), n


def test_cus_is_read_from_the_environment():
    """CNN_AMD_CUS in the environment of a fresh process, read once when the library is first used"""
    code = ("import ctypes as C; from cnn_amd import capi; d = capi.ConvDesc(%d, %d, %d, %d, %d, %d, %d, %d); "
            "print(capi.get_option('CUS'), int(capi.load().cnn_conv2d_workspace_bytes(C.byref(d))))" % C11B)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, CNN_AMD_CUS="5"), capture_output=True, text=True,
                         check=True).stdout.split()
    assert out == ["5", str(_c11b_bytes(10))], out


def test_the_prefixed_name_sets_the_same_switch(lib_option):
    lib_option("CUS", None)
    capi.set_option("CNN_AMD_CUS", "5")
    try:
        assert capi.get_option("CUS") == "5" and _ws(C11B) == _c11b_bytes(10)
    finally:
        capi.set_option("CNN_AMD_CUS", None)


def test_a_1x1_workspace_moves_with_cus(lib_option):
    lib_option("CUS", None)
    own = _ws(C11)
    assert own == ((49 + 1) * 64 * 65 + 64) * 4  # 49 slabs of Co x (Ci + 1) floats, one slab row of reduction scratch
    lib_option("CUS", "1")
    assert _ws(C11) < own


def test_no_memo_answers_for_another_cu_count(lib_option):
    """DescMemo / RouteFacts key on the option generation and on num_cus(): unset -> CUS=1 -> unset gives first == third != second,
    at once and after 20 other descs have gone through the 16-entry rings"""
    lib_option("CUS", None)
    first = {c: _sizes(c) for c in (STEM, C11)}
    lib_option("CUS", "1")
    second = {c: _sizes(c) for c in (STEM, C11)}
    lib_option("CUS", None)
    assert {c: _sizes(c) for c in (STEM, C11)} == first
    assert all(second[c][0] < first[c][0] for c in first)
    others = [c for c in R.HAND_PICKED if c not in (STEM, C11)][:20]
    assert len(others) == 20
    lib_option("CUS", "1")
    small = {c: _sizes(c) for c in others}
    assert {c: _sizes(c) for c in (STEM, C11)} == second
    lib_option("CUS", None)
    plain = {c: _sizes(c) for c in others}
    assert {c: _sizes(c) for c in (STEM, C11)} == first
    lib_option("CUS", "1")
    assert {c: _sizes(c) for c in others} == small and {c: _sizes(c) for c in (STEM, C11)} == second
    lib_option("CUS", None)
    assert {c: _sizes(c) for c in others} == plain
    assert any(small[c] != plain[c] for c in others)  # (the 20 descs are no bystanders: some of their sizes move too)


def test_route_sizes_are_unchanged_without_cus(lib_option):
    """tests/golden/conv_route_sizes.json (test_conv_route_sizes.py) still holds after CUS has been set, used and removed in this process"""
    from tests.test_conv_route_sizes import test_conv_sizes_and_predicates_match_the_recorded_ones as recorded_sizes_hold

    lib_option("CUS", "5")
    for c in R.HAND_PICKED:
        _sizes(c)
    lib_option("CUS", None)
    recorded_sizes_hold()
