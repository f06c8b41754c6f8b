"""No device needed: the decoys of the stream-order cases (tests/stream_order.py) do not give the real answer.  A call that read a
decoy where it should have waited for the real input must land further than 100 x REL_TOL from the reference, or the gated comparison
could pass by accident."""
import numpy as np
import pytest

from tests import conv_route_cases as R
from tests import stream_order as SO
from tests import stream_order_cases as K
from tests import streaming_cases as C
from tests.util import normal_scaled, rel_err, uniform01, uniform_pm1


@pytest.mark.parametrize("case", K.FORK_DESCS, ids=R.key)
def test_fork_and_join_decoys_are_far_from_the_reference(case):
    real, decoy = K.fork_inputs(case), K.fork_inputs(case, decoy=True)
    kinds = ["backward", "prepared_relu"] + (["pooled2"] if case == K.POOLED_DESC else [])
    for kind in kinds:
        SO.assert_decoy_differs(K.fork_reference(case, kind, real), K.fork_reference(case, kind, decoy), f"{R.key(case)} {kind}")
        # ... and one late operand alone is enough: each input of the variant replaced by its decoy on its own
        reads = {"backward": ("x", "dy", "w"), "prepared_relu": ("x", "dy", "w", "relu_below"), "pooled2": ("x", "dpool", "mask", "pooled", "w")}[kind]
        want = K.fork_reference(case, kind, real)
        for name in reads:
            got = K.fork_reference(case, kind, dict(real, **{name: decoy[name]}))
            assert any(rel_err(got[o], want[o]) > SO.DECOY_FACTOR * SO.REL_TOL for o in want), (R.key(case), kind, name)


@pytest.mark.parametrize("name", sorted(K.LAYERS))
def test_layer_decoys_are_far_from_the_reference(name):
    inputs, reference = K.LAYERS[name]
    real, decoy = reference(inputs()), reference(K.layer_decoys(name))
    as_f64 = lambda d: {k: np.asarray(v, np.float64) for k, v in d.items()}
    SO.assert_decoy_differs(as_f64(real), as_f64(decoy), name)


def test_published_kernel_decoys_are_far_from_the_reference():
    SO.assert_decoy_differs(K.published_linear_reference(K.published_linear_inputs()),
                            K.published_linear_reference(K.published_linear_inputs(decoy=True)), "published linear backward")
    SO.assert_decoy_differs(K.published_relu_reference(K.published_relu_inputs()),
                            K.published_relu_reference(K.published_relu_inputs(decoy=True)), "published relu")


def _conv_route_operands(i):
    """the operands of HAND_PICKED[i] as tests/conv_route_cases.py::_Layer seeds them, and the decoys tests/test_gpu_stream_order_conv.py
    ::_layer gives them (same seeds, same order)"""
    B, Ci, H, W, Co, k, s, pad = R.HAND_PICKED[i][:8]
    seed = 9000 + 10 * i
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    x = uniform01(seed, (B, Ci, H, W))
    real = {"x": x, "w": normal_scaled(seed + 1, (Co, Ci, k, k)), "b": normal_scaled(seed + 2, (Co,)), "dy": uniform_pm1(seed + 3, (B, Co, Ho, Wo)),
            "relu_below": np.where(x - np.float32(0.5) >= 0, x - np.float32(0.5), np.float32(0)).astype(np.float32)}
    decoy = {name: SO.decoy_of(real[name], 9500 + 10 * i + j) for j, name in enumerate(("x", "w", "b", "dy", "relu_below"))}
    return real, decoy


def _conv_route_reference(i, t):
    """what the calls of one desc compute, from the CPU oracle: forward (+ ReLU), data gradient (+ ReLU'), weight / bias gradient"""
    from oracle import pyoracle as O

    s, pad = R.HAND_PICKED[i][6:8]
    y = O.conv2d_forward_padded(t["x"], t["w"], t["b"], s, pad)
    gw, gb, dx = O.conv2d_backward_padded(t["x"], t["dy"], t["w"], s, pad)
    return {"y": y, "y_relu": np.maximum(y, 0), "dx": dx, "dx_relu": np.where(t["relu_below"] <= 0, np.float32(0), dx), "gw": gw, "gb": gb}


@pytest.mark.parametrize("i", range(len(R.HAND_PICKED)), ids=[R.key(c) for c in R.HAND_PICKED])
def test_conv_route_decoys_are_far_from_the_reference(i):
    """every desc of HAND_PICKED with the seeds and shapes of the GPU cases.  (The prepared calls' extra late operands, the filter
    images, have all-zero bytes as their decoy: a zero filter image is a zero convolution, no reference is needed for that.)"""
    from oracle import pyoracle as O

    real, decoy = _conv_route_operands(i)
    O.set_threads(0)
    try:
        SO.assert_decoy_differs(_conv_route_reference(i, real), _conv_route_reference(i, decoy), R.key(R.HAND_PICKED[i]))
    finally:
        O.set_threads(1)


def test_layerwise_decoys_are_far_from_the_reference():
    """segment norms, one LAMB and one LARS step of tests/test_gpu_stream_order_plumbing.py through tests/lamb_ref.py"""
    from tests.lamb_ref import ref_lamb_moments, ref_lamb_step, ref_lars_step, ref_segment_norms
    from tests.test_gpu_layerwise import LAMB, LARS, LR, make_data, make_flags, make_table

    n = 5
    bounds = make_table("seven", n, 45)
    flags = make_flags("mixed", len(bounds) - 1)
    p, (g,) = make_data(n, bounds, 46, 1)
    zeros = np.zeros(n, np.float32)
    real = {"p": p, "g": g, "m": zeros, "v": zeros}
    decoy = {k: SO.decoy_of(real[k], 8000 + i) for i, k in enumerate(("p", "g", "m"))}
    decoy["v"] = decoy["m"] * decoy["m"]

    def reference(t):
        wn = ref_segment_norms(t["p"], bounds)
        r, _, _ = ref_lamb_moments(t["p"], t["g"], t["m"], t["v"], bounds, flags, 1, weight_decay=1e-2, grad_scale=0.125, **LAMB)
        lp, lm, lv, lr_, _ = ref_lamb_step(t["p"], t["g"], t["m"], t["v"], bounds, flags, 1, LR, wn, ref_segment_norms(r, bounds), weight_decay=1e-2,
                                           grad_scale=0.125, **LAMB)
        gn = ref_segment_norms(t["g"], bounds) * np.float32(0.125)
        sp, sv, _, _ = ref_lars_step(t["p"], t["g"], t["m"], bounds, flags, LR, wn, gn, weight_decay=1e-2, grad_scale=0.125, norm_is_scaled=True, **LARS)
        return {"norms": wn, "lamb_p": lp, "lamb_m": lm, "lamb_v": lv, "lamb_update": lr_, "lars_p": sp, "lars_velocity": sv}

    SO.assert_decoy_differs(reference(real), reference(decoy), "layer-wise optimizers")


def test_decoys_of_the_remaining_cases_differ_from_their_inputs():
    """Input distance only, per operand, with the seeds and shapes of the GPU cases -- NOT a reference on the decoy:
    * streaming cases: held by SHA-256 digests, any differing output byte fails them; every entry is elementwise in each operand;
    * copies, memset, events, one-rank collectives and the stagers: their reference IS the operand (or its ReLU / byte conversion),
      so the distance of the operand is the distance of the reference."""
    from tests.test_gpu_stream_order_plumbing import _stager_batch

    far = lambda a, b: rel_err(a, b) > SO.DECOY_FACTOR * SO.REL_TOL
    for n in C.SMALL:
        rs = np.random.RandomState(4200 + n % 1000)
        dev = [rs.standard_normal(n).astype(np.float32) for _ in range(4)]
        decoys = [SO.decoy_of(d, 7600 + 10 * (n % 100) + k) for k, d in enumerate(dev)]
        assert all(far(d, r) for d, r in zip(decoys, dev)) and far(decoys[3] * decoys[3], dev[3] * dev[3])
    for seed, shape in ((8100, (4099,)), (8200, (100003,))):
        real = uniform_pm1(seed, shape)
        assert far(SO.decoy_of(real, seed + 1), real) and far(np.maximum(SO.decoy_of(real, seed + 1), 0), np.maximum(real, 0))
    for kind in ("f32", "u8"):
        assert far(_stager_batch(kind, 8301)[1], _stager_batch(kind, 8300)[1])


def test_first_block_im2col_and_tune_decoys_are_far_from_the_reference():
    real, decoy = K.fork_inputs(K.POOLED_DESC), K.fork_inputs(K.POOLED_DESC, decoy=True)
    SO.assert_decoy_differs(K.first_block_forward_reference(real), K.first_block_forward_reference(decoy), "first block forward")
    SO.assert_decoy_differs(K.im2col_reference(K.im2col_inputs()), K.im2col_reference(K.im2col_inputs(decoy=True)), "im2col")
    for co in K.TUNE_CO:
        SO.assert_decoy_differs(K.tune_reference(K.tune_inputs(), co), K.tune_reference(K.tune_inputs(decoy=True), co), "tile measurement")


def test_python_driver_decoys_are_far_from_the_reference():
    from tests.test_gpu_stream_order_pynet import decoys, inputs, oracle_steps

    SO.assert_decoy_differs(oracle_steps(inputs()), oracle_steps(decoys()), "three steps of the Python driver")


def test_container_decoys_differ_from_their_inputs():
    """input distance only: the container cases compare digests of parameters, gradients and every layer's output after three or
    four train steps; the decoy batch is far from the real one and every decoy label is wrong"""
    import zlib

    from tests import host_layer_cases as L
    from tests.test_gpu_stream_order_container import CONTAINER_CASES

    for name in CONTAINER_CASES:
        _, in_shape, B = L.NETS[L.CASES[name][0]]
        x = uniform01(7000 + zlib.crc32(name.encode()) % 1000, (B,) + in_shape)
        assert rel_err(SO.decoy_of(x, 7801), x) > SO.DECOY_FACTOR * SO.REL_TOL
        labels = np.arange(B) % 3
        assert np.all((labels + 1) % 3 != labels)
