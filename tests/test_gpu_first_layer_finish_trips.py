"""first_layer_finish (the one-workgroup end of the first layer's step: slab sum -> gradient -> SGD -> kept copy -> both filter images)
at every slab count where its batched slab loads change shape, against the unfused sequence cnn_conv2d_backward_weight_pooled2
(weight gradient + slab reduction) + cnn_sgd_update + cnn_conv2d_prepare_filters: gw, gb, w, bias, the kept copies and both filter
images bit for bit.

The slab count is the window kernel's grid (win_wgrad_slots, conv_wgrad_win.hip): min(ceil(strips / 8), CUs) with
strips = B * ceil(Ho / 2) * ceil(ceil(Wo / 2) / 16).  A 19 x 19 image has Ho = Wo = 9: 5 strips per sample; 224 x 224 has
Ho = Wo = 111: 56 * 4 = 224 strips per sample.  The kernel sums in eight slot-lanes and loads 16 rounds of them (128 slots) per batch:

    (B, H, W)         strips   slabs
    (1, 19, 19)            5       1    one slot-lane live
    (5, 19, 19)           25       4    fewer than eight
    (12, 19, 19)          60       8    every slot-lane once
    (13, 19, 19)          65       9    a second round, one lane
    (100, 19, 19)        500      63    one short of 64 slots
    (102, 19, 19)        510      64
    (103, 19, 19)        515      65
    (204, 19, 19)      1 020     128    exactly one batch
    (205, 19, 19)      1 025     129    the second batch, one slot
    (10, 224, 224)     2 240     CUs    the whole chip (256 slabs on an MI355X: two batches)
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import normal_scaled, uniform_pm1

pytestmark = pytest.mark.gpu

# (B, H, W) -> slabs; None = the device's CU count
GEOMETRIES = [((1, 19, 19), 1), ((5, 19, 19), 4), ((12, 19, 19), 8), ((13, 19, 19), 9), ((100, 19, 19), 63), ((102, 19, 19), 64),
              ((103, 19, 19), 65), ((204, 19, 19), 128), ((205, 19, 19), 129), ((10, 224, 224), None)]


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    arch = capi.load().cnn_amd_device_arch().decode()
    assert arch == "gfx950", f"built for gfx950, running on {arch}"
    return torch


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def slabs_of(T, B, H, W):
    """win_wgrad_slots' rule, restated"""
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    WR, WC = (Ho + 1) // 2, (Wo + 1) // 2
    strips = B * WR * ((WC + 15) // 16)
    return min((strips + 7) // 8, T.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("shape,slabs", GEOMETRIES, ids=lambda v: "B%d_%dx%d" % v if isinstance(v, tuple) else f"slabs_{v or 'CUs'}")
def test_fused_step_end_is_bit_identical_at_every_slab_count(T, shape, slabs):
    from cnn_amd import capi

    B, H, W = shape
    cus = T.cuda.get_device_properties(0).multi_processor_count
    assert slabs_of(T, B, H, W) == (cus if slabs is None else slabs), "the geometry no longer gives the slab count it is here for"
    conv = capi.Conv2d(B, 3, H, W, 16, 3, 2, 0)
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    PHo, PWo = Ho // 2, Wo // 2
    xd = dev(T, uniform_pm1(970, (B, 3, H, W)))
    wd, bd = dev(T, normal_scaled(971, (16, 3, 3, 3))), dev(T, normal_scaled(972, (16,)))
    pooled = T.empty((B, 16, PHo, PWo), device="cuda")
    mask = T.empty((B, 16, PHo, PWo), dtype=T.int32, device="cuda")
    conv.relu_maxpool2_forward(xd, wd, bd, pooled, mask)
    dpool = dev(T, uniform_pm1(973, (B, 16, PHo, PWo)))
    lr, scale = 0.05, 0.5
    # the unfused sequence
    gw_ref, gb_ref = T.empty_like(wd), T.empty_like(bd)
    conv.backward_weight_pooled2(xd, dpool, mask, pooled, float(B), gw_ref, gb_ref)
    w_ref, b_ref = wd.clone(), bd.clone()
    capi.sgd_update(w_ref.view(-1), gw_ref.view(-1), lr, scale)
    capi.sgd_update(b_ref, gb_ref, lr, scale)
    pf_ref, pd_ref = conv.prepared_buffers("cuda")
    pf_ref.zero_(); pd_ref.zero_()
    capi.prepare_filters([conv], [w_ref], [b_ref], [pf_ref], [pd_ref])
    # the fused step end
    gw, gb, w2, b2 = T.full_like(wd, 7.0), T.full_like(bd, 7.0), wd.clone(), bd.clone()
    w_kept, b_kept = T.full_like(wd, 7.0), T.full_like(bd, 7.0)
    pf, pd = conv.prepared_buffers("cuda")
    pf.zero_(); pd.zero_()
    P = capi._ptr
    capi.check(conv.lib.cnn_conv2d_backward_weight_pooled2_sgd_keep(C.byref(conv.desc), P(xd), P(dpool), P(mask), P(pooled), P(gw), P(gb), float(B),
                                                                    P(w2), P(b2), lr, scale, P(pf), P(pd), P(w_kept), P(b_kept), P(conv.ws),
                                                                    conv.ws_bytes, capi._stream()), "cnn_conv2d_backward_weight_pooled2_sgd_keep")
    T.cuda.synchronize()
    nf, nd = 28 * 16, 16 * 32  # floats of the two images (conv_direct.hip: [tap | bias][co], [co][32])
    for name, a, c in (("gw", gw_ref, gw), ("gb", gb_ref, gb), ("w", w_ref, w2), ("bias", b_ref, b2), ("kept w", wd, w_kept),
                       ("kept bias", bd, b_kept)):
        assert np.array_equal(u32(a), u32(c)), name
    assert np.array_equal(u32(pf).ravel()[:nf], u32(pf_ref).ravel()[:nf]), "forward filter image"
    assert np.array_equal(u32(pd).ravel()[:nd], u32(pd_ref).ravel()[:nd]), "data-gradient filter image"
    assert not np.array_equal(u32(w2), u32(wd))
