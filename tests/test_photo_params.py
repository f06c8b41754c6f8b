"""hostapi.photo_params: the host-side sampler of a batch's photometric parameters (colour jitter as ColorJitter samples it, one erase
box as timm's RandomErasing samples it).  Host only, no device."""
import numpy as np
import pytest

from cnn_amd import capi, hostapi

B, H, W = 64, 32, 40


def boxes(p):
    return p[:, 12:16]


def test_the_sampler_is_deterministic_per_seed():
    a = hostapi.photo_params(np.random.default_rng(3), B, H, W, hue=0.05, erase_prob=0.5, erase_value="rand")
    b = hostapi.photo_params(np.random.default_rng(3), B, H, W, hue=0.05, erase_prob=0.5, erase_value="rand")
    c = hostapi.photo_params(np.random.default_rng(4), B, H, W, hue=0.05, erase_prob=0.5, erase_value="rand")
    assert a.dtype == np.float32 and a.shape == (B, 20) and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert not a[:, 19].any() and np.isfinite(a).all()
    assert len({r.tobytes() for r in a[:, :12]}) == B  # every sample its own colour map


@pytest.mark.parametrize("value", ["const", "rand"])
def test_every_box_fits_and_has_whole_number_fields(value):
    p = hostapi.photo_params(np.random.default_rng(5), 256, H, W, erase_prob=0.5, erase_value=value)
    bx = boxes(p)
    assert np.array_equal(bx, np.floor(bx)) and (bx >= 0).all()
    has = bx[:, 2] > 0
    assert 0 < has.sum() < 256  # asked of the sample itself: some with a box, some without
    assert ((bx[:, 3] > 0) == has).all()
    assert (bx[has, 0] + bx[has, 2] <= W).all() and (bx[has, 1] + bx[has, 3] <= H).all()
    assert (bx[has, 2] < W).all() and (bx[has, 3] < H).all()
    area = bx[has, 2] * bx[has, 3] / (H * W)
    aspect = bx[has, 3] / bx[has, 2]
    # (the rounding of w and h moves a small box's area and aspect by up to half a pixel per side)
    assert area.min() > 0.02 * 0.5 and area.max() < (1 / 3) * 1.2 and aspect.min() > 0.3 / 1.5 and aspect.max() < 3.3 * 1.5
    assert not p[~has, 12:19].any()
    if value == "const":
        assert not p[:, 16:19].any()
    else:
        assert (p[has, 16:19] != 0).all() and len(np.unique(p[has, 16:19])) == 3 * has.sum()


def test_erase_probability_zero_and_one():
    none = hostapi.photo_params(np.random.default_rng(6), B, H, W, erase_prob=0.0)
    assert not boxes(none).any()
    every = hostapi.photo_params(np.random.default_rng(6), B, H, W, erase_prob=1.0)
    assert (boxes(every)[:, 2] > 0).all() and (boxes(every)[:, 3] > 0).all()


def test_colour_factors_stay_within_their_ranges():
    """one op at a time, so that the factor can be read back from the map"""
    eye = np.eye(3, dtype=np.float32)
    tol = 1e-6
    p = hostapi.photo_params(np.random.default_rng(7), B, H, W, brightness=0.4, contrast=0, saturation=0, erase_prob=0)
    f = p[:, 0]
    assert np.array_equal(p[:, :9].reshape(B, 3, 3), f[:, None, None] * eye) and not p[:, 9:12].any()
    assert f.min() >= 0.6 - tol and f.max() <= 1.4 + tol and f.max() - f.min() > 0.4
    p = hostapi.photo_params(np.random.default_rng(7), B, H, W, brightness=0, contrast=0.3, saturation=0, pivot=0.25, erase_prob=0)
    f = p[:, 0]
    assert np.array_equal(p[:, :9].reshape(B, 3, 3), f[:, None, None] * eye)
    assert f.min() >= 0.7 - tol and f.max() <= 1.3 + tol and f.max() - f.min() > 0.3
    assert np.allclose(p[:, 9:12], ((1 - f.astype(np.float64)) * 0.25)[:, None], rtol=0, atol=tol)
    p = hostapi.photo_params(np.random.default_rng(7), B, H, W, brightness=0, contrast=0, saturation=1.5, erase_prob=0)
    f = (p[:, [0, 4, 8]].astype(np.float64).sum(axis=1) - 1) / 2  # trace = 3 f + (1 - f)
    assert f.min() >= 0.0 - tol and f.max() <= 2.5 + tol and f.max() - f.min() > 1.0  # (the lower end is max(0, 1 - a))
    assert np.allclose(p[:, :9].reshape(B, 3, 3).sum(axis=2), 1.0, rtol=0, atol=1e-6)  # rows of a saturation map sum to 1
    p = hostapi.photo_params(np.random.default_rng(7), B, H, W, brightness=0, contrast=0, saturation=0, hue=0.1, erase_prob=0)
    A = p[:, :9].reshape(B, 3, 3).astype(np.float64)
    yiq = np.array([[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]])
    rot = yiq @ A @ np.linalg.inv(yiq)  # back in YIQ: [[1, 0, 0], [0, cos, -sin], [0, sin, cos]]
    angle = np.degrees(np.arctan2(rot[:, 2, 1], rot[:, 1, 1]))
    assert np.abs(angle).max() <= 36.0 + 1e-3 and angle.max() > 10 and angle.min() < -10
    # nothing asked for: the identity block
    p = hostapi.photo_params(np.random.default_rng(7), 3, H, W, brightness=0, contrast=0, saturation=0, erase_prob=0)
    assert np.array_equal(p, np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1] + [0] * 11, np.float32), (3, 1)))


def test_bad_arguments_are_refused():
    with pytest.raises(capi.CnnAmdError, match="erase_value"):
        hostapi.photo_params(np.random.default_rng(1), 2, H, W, erase_value="pixel")
    with pytest.raises(capi.CnnAmdError, match="hue"):
        hostapi.photo_params(np.random.default_rng(1), 2, H, W, hue=0.7)
