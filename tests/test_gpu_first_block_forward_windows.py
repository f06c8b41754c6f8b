"""The fused first block (cnn_conv2d_relu_maxpool2_forward, kernel conv_fwd_pool_pk_3_16_3_2) with one lane per pooling window
(profiles/first_block_forward.md): pooled values, int32 mask, packed one-byte mask and the mask = NULL call against
cnn_conv2d_forward_relu + cnn_maxpool2d_forward -- other kernels -- bit for bit, from plain and prepared filters, and the lane-pair
body (CNN_AMD_FWD_POOL_PAIR=1) against the same reference.  Shapes are the places where the window -> lane mapping can break."""
import numpy as np
import pytest

from tests.util import normal_scaled, uniform01

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 7, 7),      # one window, 63 lanes without one
    (5, 7, 5),      # no last-column pair, the image stride with B > 1
    (3, 37, 41),    # W no multiple of 4 (rows of 20 bytes at any 4-byte alignment), odd Ho / Wo, 72 windows = a full item + a ragged one
    (2, 70, 66),    # 17 x 16 = 272 windows = 4.25 items: rows of windows straddle item boundaries
    (2, 12, 270),   # one row of windows (67) longer than a wave
    (2, 224, 224),  # the real plane: 47.3 items per image
]


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    assert capi.load().cnn_amd_device_arch().decode() == "gfx950"
    return torch


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.uint32)


def check_all_forms(T, lib_option, x, w, b):
    """every form of the fused call == the two-kernel reference (computed once); returns (pooled, marked int32 mask, mask bytes) of it"""
    from cnn_amd import capi

    B, _, H, W = x.shape
    case = (B, 3, H, W, 16, 3, 2, 0)
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    PHo, PWo = Ho // 2, Wo // 2
    pitch = (PWo + 3) & ~3
    xd, wd, bd = dev(T, x), dev(T, w), dev(T, b)
    conv, packed = capi.Conv2d(*case), capi.Conv2d(*case)
    assert conv.relu_maxpool2_supported() and packed.pool_mask_packed_supported()
    packed.set_pool_mask_packed()
    y, r = T.empty((B, 16, Ho, Wo), device="cuda"), T.empty((B, 16, Ho, Wo), device="cuda")
    conv.forward_relu(xd, wd, bd, y, r)
    pooled_ref, mask_ref = capi.maxpool_forward(r, 2, 2)
    want_pooled = bits(pooled_ref)
    # bit 31 marks exactly the windows whose pooled value is <= 0; the rest is cnn_maxpool2d_forward's flat index
    want_mask = host(mask_ref).astype(np.uint32) | np.where(host(pooled_ref) <= 0, np.uint32(0x80000000), np.uint32(0))
    pf, pd = conv.prepared_buffers("cuda")
    capi.prepare_filters([conv], [wd], [bd], [pf], [pd])
    n8 = B * 16 * PHo * pitch
    assert packed.pool_mask_bytes() == n8 + 64
    bytes_seen = None
    for pair in (None, "1"):  # the window body (default), the lane-pair body
        lib_option("FWD_POOL_PAIR", pair)
        for prep in (None, pf):
            tag = (pair, prep is not None)
            pooled = T.full_like(pooled_ref, 7.0)
            mask = T.full_like(mask_ref, -1)
            conv.relu_maxpool2_forward(xd, wd, bd, pooled, mask, prepared_fwd=prep)
            assert np.array_equal(bits(pooled), want_pooled), tag
            assert np.array_equal(host(mask).view(np.uint32), want_mask), tag
            pooled0 = T.full_like(pooled_ref, 7.0)  # mask = NULL
            conv.relu_maxpool2_forward(xd, wd, bd, pooled0, None, prepared_fwd=prep)
            assert np.array_equal(bits(pooled0), want_pooled), tag
            pooled8 = T.full_like(pooled_ref, 7.0)
            mask8 = T.full((n8 + 64,), 0x55, dtype=T.uint8, device="cuda")
            packed.relu_maxpool2_forward(xd, wd, bd, pooled8, mask8, prepared_fwd=prep)
            assert np.array_equal(bits(pooled8), want_pooled), tag
            m8 = host(mask8)
            rows = m8[:n8].reshape(B, 16, PHo, pitch)
            assert np.all(rows[..., PWo:] == 0x55) and np.all(m8[n8:] == 0x55), tag  # pad bytes / slack are never written
            assert np.all((rows[..., :PWo] & 0x7C) == 0), tag
            unpacked = T.full_like(mask_ref, -2)
            packed.pool_mask_unpack(mask8, unpacked)
            assert np.array_equal(host(unpacked).view(np.uint32), want_mask), tag
            if bytes_seen is None:
                bytes_seen = rows[..., :PWo].copy()
            assert np.array_equal(rows[..., :PWo], bytes_seen), tag  # old body == new body == both filter forms, byte for byte
    lib_option("FWD_POOL_PAIR", None)
    return host(pooled_ref), want_mask, bytes_seen


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_%dx%d" % s)
def test_window_per_lane_forward_is_bit_identical(T, lib_option, shape):
    """x - 0.5: many windows that are all zero after the ReLU (first maximum wins), plus NaN and inf inputs"""
    B, H, W = shape
    x = uniform01(700, (B, 3, H, W)) - np.float32(0.5)
    if H >= 12 and W >= 12:
        x[0, :, 4:9, 4:9] = np.nan
        x[-1, 1, 10, 11] = np.inf
    else:
        x[0, 1, 2, 2] = np.nan
        x[-1, 2, 3, 3] = np.inf
    w, b = normal_scaled(701, (16, 3, 3, 3)), normal_scaled(702, (16,))
    pooled, mask, _ = check_all_forms(T, lib_option, x, w, b)
    if H >= 12:
        assert np.any(pooled == 0) and np.any(pooled > 0)  # (both kinds of window are there)


def test_zero_inputs_negative_weights_minus_zero_bias(T, lib_option):
    """products of -0 on a region of exact zeros, bias -0.0: fma(w, 0, +0) is +0 and +0 + -0 is +0, so these windows pool to +0"""
    B, H, W = 3, 37, 41
    x = uniform01(710, (B, 3, H, W)) - np.float32(0.5)
    x[:, :, 8:30, 6:33] = 0.0
    x[1] = 0.0
    w = -np.abs(normal_scaled(711, (16, 3, 3, 3))) - np.float32(0.01)
    b = np.full((16,), -0.0, np.float32)
    pooled, mask, _ = check_all_forms(T, lib_option, x, w, b)
    assert np.all(pooled[1].view(np.uint32) == 0) and np.all(mask[1] >> 31 == 1)


def test_all_zero_weights_signed_zero_bias_four_way_ties(T, lib_option):
    """every window is a four-way tie of zeros: first pixel wins, and the pooled sign bits are the reference's"""
    B, H, W = 2, 37, 41
    x = uniform01(720, (B, 3, H, W)) - np.float32(0.5)
    w = np.zeros((16, 3, 3, 3), np.float32)
    b = np.where(np.arange(16) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    pooled, mask, codes = check_all_forms(T, lib_option, x, w, b)
    assert np.all(pooled == 0) and np.all(codes == 0x80)


def test_all_negative_preactivations(T, lib_option):
    """pooled +0 everywhere, the mask names the window's first pixel and carries the mark"""
    B, H, W = 2, 70, 66
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    x = uniform01(730, (B, 3, H, W)) + np.float32(0.1)
    w = -np.abs(normal_scaled(731, (16, 3, 3, 3))) - np.float32(0.01)
    b = -np.abs(normal_scaled(732, (16,))) - np.float32(0.01)
    pooled, mask, codes = check_all_forms(T, lib_option, x, w, b)
    assert np.all(pooled.view(np.uint32) == 0) and np.all(codes == 0x80)
    ph, pw = np.meshgrid(np.arange(Ho // 2), np.arange(Wo // 2), indexing="ij")
    first = (np.arange(16)[:, None, None] * Ho * Wo + 2 * ph * Wo + 2 * pw).astype(np.uint32) | np.uint32(0x80000000)
    assert np.array_equal(mask, np.broadcast_to(first, mask.shape))
