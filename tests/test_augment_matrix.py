"""cnn_augment_matrix (include/cnn_amd.h) and hostapi.augment_params: composing the per-sample output -> source maps of cnn_augment_u8
on the host.  No device calls.  The exact cases are compared with ==; the closed forms are evaluated in double and rounded to float32
once, as the entry point does."""
import numpy as np
import pytest

from cnn_amd import capi, hostapi

H, F, C_, R = capi.AUG_HFLIP, capi.AUG_VFLIP, capi.AUG_CROP, capi.AUG_ROTATE


def mat(ops, Hs, Ws, Ho, Wo):
    m = capi.augment_matrix(ops, Hs, Ws, Ho, Wo)
    assert m.dtype == np.float32 and m.shape == (6,)
    return m.tolist()


def f32(*vals):
    return [float(np.float32(v)) for v in vals]


def test_identity_and_flips_are_exact():
    assert mat([], 7, 9, 7, 9) == [1, 0, 0, 0, 1, 0]
    assert mat([(H,)], 7, 9, 7, 9) == [-1, 0, 8, 0, 1, 0]  # {-1, 0, Ws-1, 0, 1, 0}
    assert mat([(F,)], 7, 9, 7, 9) == [1, 0, 0, 0, -1, 6]
    assert mat([(H,), (H,)], 7, 9, 7, 9) == [1, 0, 0, 0, 1, 0]
    assert mat([(F,), (H,), (F,), (H,)], 7, 9, 7, 9) == [1, 0, 0, 0, 1, 0]


def test_quarter_turns_on_a_square_canvas_are_exact():
    """positive = counter-clockwise on the screen: out[y][x] = src[x][N-1-y] for 90 degrees, which is np.rot90"""
    N = 6
    assert mat([(R, 90.0)], N, N, N, N) == [0, -1, N - 1, 1, 0, 0]
    assert mat([(R, 180.0)], N, N, N, N) == [-1, 0, N - 1, 0, -1, N - 1]
    assert mat([(R, 270.0)], N, N, N, N) == [0, 1, 0, -1, 0, N - 1]
    assert mat([(R, -90.0)], N, N, N, N) == mat([(R, 270.0)], N, N, N, N)
    assert mat([(R, 360.0)], N, N, N, N) == [1, 0, 0, 0, 1, 0] == mat([(R, 0.0)], N, N, N, N)
    assert mat([(R, 90.0)] * 4, N, N, N, N) == [1, 0, 0, 0, 1, 0]
    img = np.arange(N * N).reshape(N, N)
    m = mat([(R, 90.0)], N, N, N, N)
    ys, xs = np.mgrid[0:N, 0:N]
    got = img[(m[3] * xs + m[4] * ys + m[5]).astype(int), (m[0] * xs + m[1] * ys + m[2]).astype(int)]
    assert np.array_equal(got, np.rot90(img))


def test_general_rotation_is_the_inverse_of_opencvs_forward_matrix():
    deg, Hs, Ws = 30.0, 7, 9
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    cx, cy = (Ws - 1) / 2, (Hs - 1) / 2
    # cv::getRotationMatrix2D(center, deg, 1): [[c, s, (1-c)*cx - s*cy], [-s, c, s*cx + (1-c)*cy]]; warpAffine applies its inverse
    fwd = np.array([[c, s, (1 - c) * cx - s * cy], [-s, c, s * cx + (1 - c) * cy], [0, 0, 1]])
    want = np.linalg.inv(fwd)[:2].reshape(-1)
    got = np.array(mat([(R, deg)], Hs, Ws, Hs, Ws))
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()


def test_resize_and_crop_then_resize_follow_the_closed_form():
    """sx = (x + 0.5) * cw / W - 0.5 (+ x0 for a crop)"""
    Hs, Ws, Ho, Wo = 7, 9, 8, 12
    assert mat([], Hs, Ws, Ho, Wo) == f32(Ws / Wo, 0, 0.5 * (Ws / Wo) - 0.5, 0, Hs / Ho, 0.5 * (Hs / Ho) - 0.5)
    x0, y0, w, h = 1, 2, 4, 3
    kx, ky = w / Wo, h / Ho
    assert mat([(C_, x0, y0, w, h)], Hs, Ws, Ho, Wo) == f32(kx, 0, 0.5 * kx - 0.5 + x0, 0, ky, 0.5 * ky - 0.5 + y0)
    # a crop of the whole canvas is no crop
    assert mat([(C_, 0, 0, Ws, Hs)], Hs, Ws, Ho, Wo) == mat([], Hs, Ws, Ho, Wo)


def test_op_order_matters():
    """an off-centre box: crop then flip shows source columns 1..4 mirrored, flip then crop shows columns 4..7 mirrored"""
    Hs, Ws = 7, 9
    box = (C_, 1, 2, 4, 3)
    crop_flip = mat([box, (H,)], Hs, Ws, 3, 4)
    flip_crop = mat([(H,), box], Hs, Ws, 3, 4)
    assert crop_flip == [-1, 0, 4, 0, 1, 2]  # x = 0 reads source column 1 + 3
    assert flip_crop == [-1, 0, 7, 0, 1, 2]  # x = 0 reads source column 8 - 1
    assert crop_flip != flip_crop
    # a second crop is placed in the first one's canvas
    assert mat([box, (C_, 1, 1, 2, 2)], Hs, Ws, 2, 2) == [1, 0, 2, 0, 1, 3]


@pytest.mark.parametrize("ops, Hs, Ws, Ho, Wo, word", [
    ([(C_, 6, 0, 4, 3)], 7, 9, 7, 9, "outside"),            # x0 + w > Ws
    ([(C_, 0, 5, 4, 3)], 7, 9, 7, 9, "outside"),            # y0 + h > Hs
    ([(C_, -1, 0, 4, 3)], 7, 9, 7, 9, "outside"),
    ([(C_, 0, 0, 0, 3)], 7, 9, 7, 9, "outside"),            # empty box
    ([(C_, 0, 0, 4, 3), (C_, 0, 0, 5, 3)], 7, 9, 7, 9, "outside"),  # fits the source but not the cropped canvas
    ([(7,)], 7, 9, 7, 9, "unknown kind"),
    ([(0,)], 7, 9, 7, 9, "unknown kind"),
    ([(R, float("nan"))], 7, 9, 7, 9, "not finite"),
    ([(R, float("inf"))], 7, 9, 7, 9, "not finite"),
    ([(C_, 0, 0, float("inf"), 3)], 7, 9, 7, 9, "not finite"),
    ([(C_, float("nan"), 0, 4, 3)], 7, 9, 7, 9, "not finite"),
    ([], 0, 9, 7, 9, "1..8192"),
    ([], 7, 9, 7, 8193, "1..8192"),
    ([], 7, -1, 7, 9, "1..8192"),
])
def test_rejected_inputs_return_a_status_and_a_message(ops, Hs, Ws, Ho, Wo, word):
    lib = capi.load()
    import ctypes as C

    arr = (capi.AugmentOp * max(len(ops), 1))(*[capi.AugmentOp(int(o[0]), *[float(v) for v in o[1:]]) for o in ops])
    m = (C.c_float * 6)()
    assert lib.cnn_augment_matrix(arr, len(ops), Hs, Ws, Ho, Wo, m) == 1  # CNN_AMD_E_BADARG
    assert word.encode() in lib.cnn_amd_last_error(), lib.cnn_amd_last_error()
    with pytest.raises(capi.CnnAmdError):
        capi.augment_matrix(ops, Hs, Ws, Ho, Wo)


def test_null_pointers_are_refused():
    lib = capi.load()
    import ctypes as C

    m = (C.c_float * 6)()
    assert lib.cnn_augment_matrix(None, 1, 7, 9, 7, 9, m) == 1 and b"null" in lib.cnn_amd_last_error()
    assert lib.cnn_augment_matrix(None, 0, 7, 9, 7, 9, None) == 1 and b"null" in lib.cnn_amd_last_error()
    assert lib.cnn_augment_matrix(None, 0, 7, 9, 7, 9, m) == 0  # (no ops: nothing to read)


def test_augment_u8_checks_its_arguments_before_any_device_call():
    lib = capi.load()
    import ctypes as C

    buf = C.create_string_buffer(64)  # (never read: every call below is refused first)
    p = C.cast(buf, C.c_void_p)
    for args, word in [((None, 1, 7, 9, p, 0.0, p, 7, 9), b"null"), ((p, 1, 7, 9, None, 0.0, p, 7, 9), b"null"),
                       ((p, 1, 7, 9, p, 0.0, None, 7, 9), b"null"), ((p, 0, 7, 9, p, 0.0, p, 7, 9), b"1..8192"),
                       ((p, 1, 7, 8193, p, 0.0, p, 7, 9), b"1..8192"), ((p, 1, 7, 9, p, 0.0, p, -3, 9), b"1..8192"),
                       ((p, 1, 7, 9, p, float("nan"), p, 7, 9), b"fill"), ((p, 1, 7, 9, p, float("-inf"), p, 7, 9), b"fill")]:
        assert lib.cnn_augment_u8(*args, None) == 1, args  # CNN_AMD_E_BADARG
        assert word in lib.cnn_amd_last_error(), (args, lib.cnn_amd_last_error())
    assert lib.cnn_batch_stager_create_u8_aug(None, 4, 7, 9, 7, 9, 2) == 1
    h = C.c_void_p()
    assert lib.cnn_batch_stager_create_u8_aug(C.byref(h), 4, 7, 9, 0, 9, 2) == 1 and b"1..8192" in lib.cnn_amd_last_error()
    assert lib.cnn_batch_stager_create_u8_aug(C.byref(h), 4, 7, 9, 7, 9, 1) == 1 and b"depth" in lib.cnn_amd_last_error()
    assert not h.value


def test_augment_params_is_reproducible_and_all_zero_probabilities_give_the_resize_map():
    a = hostapi.augment_params(np.random.default_rng(7), 16, 60, 80, 32, 48)
    b = hostapi.augment_params(np.random.default_rng(7), 16, 60, 80, 32, 48)
    c = hostapi.augment_params(np.random.default_rng(8), 16, 60, 80, 32, 48)
    assert a.shape == (16, 6) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert len({tuple(r) for r in a.tolist()}) > 8  # the samples of a batch differ
    none = hostapi.augment_params(np.random.default_rng(7), 5, 60, 80, 32, 48, hflip=0, vflip=0, crop=0, rotate=0)
    assert np.array_equal(none, np.tile(capi.augment_matrix([], 60, 80, 32, 48), (5, 1)))
    # all probabilities 1, no rotation range, full-size crop: flips only, whatever the order
    flips = hostapi.augment_params(np.random.default_rng(1), 4, 7, 9, 7, 9, hflip=1, vflip=1, crop=1, rotate=1, crop_min=1.0, max_angle=0.0)
    assert np.array_equal(flips, np.tile(np.array([-1, 0, 8, 0, -1, 6], np.float32), (4, 1)))
