"""cnn_colour_matrix (include/cnn_amd.h) through capi.colour_matrix: host only, no device.  Each op and composed lists against a float64
NumPy restatement of the header's formulas.  Tolerance: one fp32 ulp of the restated value per entry -- the library composes in double and
rounds to fp32 once, so it can differ from a double restatement (whose operations may run in another order: their ~1e-16 differences
are 1e-9 of an fp32 ulp) only where the double value sits at a rounding tie."""
import ctypes as C

import numpy as np
import pytest

from cnn_amd import capi

GRAY = np.array([0.299, 0.587, 0.114])
YIQ = np.array([[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]])


def ref_op(kind, a, b=0.0):
    """-> (L 3x3, k 3) of x -> L x + k, float64"""
    a, b = float(np.float32(a)), float(np.float32(b))  # (the ABI carries fp32 arguments)
    if kind == capi.COL_BRIGHTNESS:
        return a * np.eye(3), np.zeros(3)
    if kind == capi.COL_CONTRAST:
        return a * np.eye(3), np.full(3, (1 - a) * b)
    if kind == capi.COL_SATURATION:
        return a * np.eye(3) + (1 - a) * np.outer(np.ones(3), GRAY), np.zeros(3)
    assert kind == capi.COL_HUE
    c, s = np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a))
    rot = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.linalg.inv(YIQ) @ rot @ YIQ, np.zeros(3)


def ref(ops):
    A, o = np.eye(3), np.zeros(3)
    for op in ops:
        L, k = ref_op(*op)
        A, o = L @ A, L @ o + k
    return np.concatenate([A.reshape(-1), o])


def within_one_ulp(got, want64):
    assert got.dtype == np.float32 and got.shape == (12,)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return bool(np.all(np.abs(got.astype(np.float64) - want64) <= ulp))


def no_negative_zero(m):
    return not np.any(np.signbit(m) & (m == 0))


def test_the_empty_list_is_the_identity():
    m = capi.colour_matrix([])
    assert m.tobytes() == np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32).tobytes()


@pytest.mark.parametrize("op", [(capi.COL_BRIGHTNESS, 1.3), (capi.COL_BRIGHTNESS, 0.0), (capi.COL_CONTRAST, 0.7, 0.5), (capi.COL_CONTRAST, 1.4, 0.449),
                                (capi.COL_SATURATION, 1.25), (capi.COL_SATURATION, 0.6), (capi.COL_HUE, 30.0), (capi.COL_HUE, -100.5)],
                         ids=lambda op: "-".join(str(v) for v in op))
def test_each_op_equals_the_restatement(op):
    m = capi.colour_matrix([op])
    assert within_one_ulp(m, ref([op])) and no_negative_zero(m)


def test_the_order_of_the_ops_counts():
    ops = [(capi.COL_BRIGHTNESS, 1.2), (capi.COL_CONTRAST, 0.8, 0.5), (capi.COL_SATURATION, 1.3), (capi.COL_HUE, 25.0)]
    other = [ops[2], ops[1], ops[3], ops[0]]
    a, b = capi.colour_matrix(ops), capi.colour_matrix(other)
    assert not np.array_equal(a, b)
    assert within_one_ulp(a, ref(ops)) and within_one_ulp(b, ref(other))
    assert np.abs(ref(ops) - ref(other)).max() > 1e-3  # (the restatement tells them apart by far more than the tolerance)
    assert no_negative_zero(a) and no_negative_zero(b)
    # ColourOp structures are taken as well as tuples
    assert np.array_equal(capi.colour_matrix([capi.ColourOp(int(op[0]), *[float(v) for v in op[1:]]) for op in ops]), a)


def test_saturation_zero_gives_equal_rows():
    m = capi.colour_matrix([(capi.COL_SATURATION, 0.0)])
    A = m[:9].reshape(3, 3)
    assert np.array_equal(A[0], A[1]) and np.array_equal(A[0], A[2])
    assert np.array_equal(A[0], GRAY.astype(np.float32)) and not m[9:].any()


def test_a_full_turn_of_the_hue_is_no_turn():
    full, none = capi.colour_matrix([(capi.COL_HUE, 360.0)]), capi.colour_matrix([(capi.COL_HUE, 0.0)])
    assert within_one_ulp(full, none.astype(np.float64)) and within_one_ulp(none, ref([]))
    assert no_negative_zero(full) and no_negative_zero(none)
    # a half turn keeps grey and negates the chroma: rows still sum to 1
    half = capi.colour_matrix([(capi.COL_HUE, 180.0)])
    assert within_one_ulp(half, ref([(capi.COL_HUE, 180.0)]))


def test_no_negative_zero_where_products_cancel():
    for ops in ([(capi.COL_BRIGHTNESS, -1.0)], [(capi.COL_BRIGHTNESS, 0.0), (capi.COL_CONTRAST, -2.0, 0.0)], [(capi.COL_CONTRAST, 1.0, -0.5)]):
        assert no_negative_zero(capi.colour_matrix(ops)), ops


def test_bad_ops_are_refused_with_a_message():
    with pytest.raises(capi.CnnAmdError, match="unknown kind"):
        capi.colour_matrix([(0, 1.0)])
    with pytest.raises(capi.CnnAmdError, match="unknown kind"):
        capi.colour_matrix([(capi.COL_BRIGHTNESS, 1.0), (5, 1.0)])
    for op in ((capi.COL_BRIGHTNESS, float("nan")), (capi.COL_CONTRAST, 0.5, float("nan")), (capi.COL_SATURATION, float("inf")), (capi.COL_HUE, float("nan"))):
        with pytest.raises(capi.CnnAmdError, match="not finite"):
            capi.colour_matrix([op])
    lib = capi.load()
    out = (C.c_float * 12)()
    assert lib.cnn_colour_matrix(None, 1, out) == 1 and b"null" in lib.cnn_amd_last_error()
    assert lib.cnn_colour_matrix(None, 0, None) == 1 and b"null" in lib.cnn_amd_last_error()
