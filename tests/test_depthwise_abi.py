"""CNN_CONV2D_DEPTHWISE at the C ABI without a device: the flag's value, the size queries, which entries serve it and which refuse it
(every argument check comes before any launch), and the host-side stack vocabulary (walk / he_init / train_flops_per_image /
mobilenet_v1)."""
import ctypes as C

import numpy as np
import pytest

from cnn_amd import capi, stacks

DW = (2, 8, 14, 14, 8, 3, 1, 1, 4)  # B, Ci, H, W, Co, k, s, pad, flags


def _desc(case=DW):
    return capi.ConvDesc(*case)


def _last_error():
    return capi.load().cnn_amd_last_error().decode()


def _dummy_args(name, d):
    """an argument list for `name` from its declared signature: the desc, then non-null pointers / plausible scalars.  Nothing is ever
    dereferenced: the calls made with these must be refused by the desc check"""
    _, argtypes = capi.SIGNATURES[name]
    keep, args = [], []
    for t in argtypes:
        if t is capi._D:
            args.append(C.byref(d))
        elif t is C.c_void_p:
            args.append(C.c_void_p(0x1000))
        elif t is C.c_size_t:
            args.append(1 << 20)
        elif t is C.c_float:
            args.append(1.0)
        elif t is C.c_int:
            args.append(1)
        elif t is C.POINTER(C.c_int32):
            keep.append((C.c_int32 * 4)())
            args.append(keep[-1])
        elif t is C.POINTER(C.c_void_p):
            keep.append((C.c_void_p * 1)(C.c_void_p(0x1000)))
            args.append(keep[-1])
        else:
            raise AssertionError((name, t))
    return args, keep


def test_the_flag_is_four():
    assert capi.DEPTHWISE == 4 and capi.POOL_MASK_PACKED == 1
    assert [n for n, _ in capi.ConvDesc._fields_] == ["B", "Ci", "H", "W", "Co", "k", "s", "pad", "flags"]
    assert capi.load().cnn_amd_abi_version() == 2


def test_size_queries_serve_the_flag():
    lib = capi.load()
    d = _desc()
    ws, bws = int(lib.cnn_conv2d_workspace_bytes(C.byref(d))), int(lib.cnn_conv2d_backward_workspace_bytes(C.byref(d)))
    assert ws > 0 and bws >= ws
    # batch slabs of [C][k*k | 1] floats: at least one, at most one per sample (+ the reduction's scratch row and 64 floats of slack)
    row = 8 * 10 * 4
    assert 2 * row + 256 <= ws <= 3 * row + 256


@pytest.mark.parametrize("cus", ["1", "2", "1000"])
def test_the_slab_planner_obeys_the_cu_count(cus):
    lib = capi.load()
    d = _desc((64, 4, 14, 14, 4, 3, 1, 1, 4))
    row = 4 * 10 * 4
    with capi.option("CUS", cus):
        ws = int(lib.cnn_conv2d_workspace_bytes(C.byref(d)))
    want = min(64, -(-4 * min(int(cus), 256) // 4))    # four workgroups per CU over the C channels, at most one slab per sample
    per = -(-64 // want)
    slots = -(-64 // per)
    assert ws == (slots + -(-slots // 64)) * row + 256, (cus, ws, slots)


def test_depthwise_needs_equal_channel_counts():
    lib = capi.load()
    d = _desc((2, 8, 14, 14, 16, 3, 1, 1, 4))
    assert lib.cnn_conv2d_workspace_bytes(C.byref(d)) == 0 and "depthwise" in _last_error() and "Co == Ci" in _last_error()
    args, _ = _dummy_args("cnn_conv2d_forward", d)
    assert lib.cnn_conv2d_forward(*args) == 1 and "Co == Ci" in _last_error()  # CNN_AMD_E_BADARG


@pytest.mark.parametrize("flags", [2, 8, 6, 12])
def test_other_bits_are_still_unknown(flags):
    lib = capi.load()
    d = _desc(DW[:8] + (flags,))
    assert lib.cnn_conv2d_workspace_bytes(C.byref(d)) == 0 and "unknown desc flags" in _last_error()
    assert lib.cnn_conv2d_backward_workspace_bytes(C.byref(d)) == 0


def test_the_flag_does_not_combine_with_the_packed_pool_mask():
    d = _desc(DW[:8] + (5,))
    assert capi.load().cnn_conv2d_workspace_bytes(C.byref(d)) == 0 and "depthwise" in _last_error()


REFUSING_CALLS = [
    "cnn_conv2d_forward_prepared", "cnn_conv2d_backward_data_prepared", "cnn_conv2d_backward_data_relu_prepared",
    "cnn_conv2d_backward_prepared", "cnn_conv2d_backward_prepared_relu",
    "cnn_conv2d_pool_mask_unpack", "cnn_conv2d_relu_maxpool2_forward", "cnn_conv2d_relu_maxpool2_forward_prepared",
    "cnn_conv2d_backward_pooled2_prepared", "cnn_conv2d_backward_weight_pooled2", "cnn_conv2d_backward_weight_pooled2_sgd",
    "cnn_conv2d_backward_weight_pooled2_sgd_keep", "cnn_conv2d_backward_data_pooled2", "cnn_conv2d_backward_data_pooled2_prepared",
    "cnn_conv2d_forward_im2col", "cnn_conv2d_backward_weight_im2col", "cnn_conv2d_backward_data_im2col",
    "cnn_conv2d_autotune", "cnn_conv2d_autotune_ws", "cnn_conv2d_tune_export", "cnn_conv2d_tune_import",
]
REFUSING_QUERIES = [
    "cnn_conv2d_prepared_bytes", "cnn_conv2d_relu_maxpool2_supported", "cnn_conv2d_pool_mask_packed_supported",
    "cnn_conv2d_pool_mask_bytes", "cnn_conv2d_relu_only_supported", "cnn_conv2d_im2col_workspace_bytes",
    "cnn_conv2d_autotune_workspace_bytes",
]


def _poison_last_error():
    d = _desc(DW[:8] + (2,))
    assert capi.load().cnn_conv2d_workspace_bytes(C.byref(d)) == 0 and "depthwise" not in _last_error()


@pytest.mark.parametrize("name", REFUSING_CALLS)
def test_entries_without_a_depthwise_path_refuse_the_flag(name):
    _poison_last_error()
    d = _desc()
    args, keep = _dummy_args(name, d)
    rc = getattr(capi.load(), name)(*args)
    assert rc != 0 and "depthwise" in _last_error(), (name, rc, _last_error())


@pytest.mark.parametrize("name", REFUSING_QUERIES)
def test_queries_without_a_depthwise_path_answer_zero(name):
    _poison_last_error()
    d = _desc()
    assert getattr(capi.load(), name)(C.byref(d)) == 0 and "depthwise" in _last_error(), (name, _last_error())


def test_prepare_filters_refuses_the_flag():
    _poison_last_error()
    descs = (capi.ConvDesc * 1)(_desc())
    args, keep = _dummy_args("cnn_conv2d_prepare_filters", descs[0])
    args[0], args[1] = 1, descs
    assert capi.load().cnn_conv2d_prepare_filters(*args) != 0 and "depthwise" in _last_error()


def test_the_lists_cover_every_entry_that_takes_a_desc():
    served = {"cnn_conv2d_workspace_bytes", "cnn_conv2d_forward", "cnn_conv2d_forward_relu", "cnn_conv2d_backward_data",
              "cnn_conv2d_backward_data_relu", "cnn_conv2d_backward_weight", "cnn_conv2d_backward_weight_side",
              "cnn_conv2d_backward_workspace_bytes", "cnn_conv2d_backward"}
    takes_desc = {n for n, (_, a) in capi.SIGNATURES.items() if capi._D in a}
    assert takes_desc == served | set(REFUSING_CALLS) | set(REFUSING_QUERIES) | {"cnn_conv2d_prepare_filters"}, \
        takes_desc ^ (served | set(REFUSING_CALLS) | set(REFUSING_QUERIES) | {"cnn_conv2d_prepare_filters"})


@pytest.mark.parametrize("case", [(1, 1 << 15, 256, 256, 1 << 15, 3, 1, 1, 4),     # x and y: 2^31 elements
                                  (1, 1 << 16, 183, 183, 1 << 16, 3, 1, 1, 4),     # 65536 * 33489 > 2^31
                                  (2, 1 << 15, 362, 362, 1 << 15, 3, 2, 1, 4)])    # x: 2^16 * 131044 > 2^31, y under it
def test_tensors_of_two_to_the_31_elements_are_refused_without_a_device(case):
    lib = capi.load()
    d = _desc(case)
    assert case[0] * case[1] * case[2] * case[3] >= 1 << 31
    _poison_last_error()
    args, _ = _dummy_args("cnn_conv2d_forward", d)
    assert lib.cnn_conv2d_forward(*args) == 1 and "2^31" in _last_error() and "depthwise" in _last_error()
    assert lib.cnn_conv2d_workspace_bytes(C.byref(d)) == 0
    for name in ("cnn_conv2d_backward_data", "cnn_conv2d_backward_weight", "cnn_conv2d_backward"):
        args, _ = _dummy_args(name, d)
        assert getattr(lib, name)(*args) == 1 and "2^31" in _last_error(), name
    under = _desc((1, 1 << 15, 255, 256, 1 << 15, 3, 1, 1, 4))
    assert lib.cnn_conv2d_workspace_bytes(C.byref(under)) > 0


# ---- the stack vocabulary -----------------------------------------------------------------------------------------------------------
SPEC = [("conv", 8, 3, 2, 1), ("relu",), ("dwconv", 5, 2, 2), ("relu",), ("linear", 3)]


def test_walk_he_init_and_flops_agree_on_dwconv():
    layout = stacks.walk(SPEC, 3, 33, 29)
    conv, _, dw, _, lin = layout
    assert conv["out"] == (8, 17, 15)
    assert dw["kind"] == "dwconv" and dw["in"] == (8, 17, 15) and dw["out"] == (8, 9, 8) and dw["params"] == 8 * 25 + 8
    assert (dw["k"], dw["s"], dw["pad"]) == (5, 2, 2) and "Co" not in dw
    assert lin["n_in"] == 8 * 9 * 8
    flat = stacks.he_init(layout, 5)
    assert flat.size == sum(e["params"] for e in layout) and flat.dtype == np.float32
    off = conv["params"]
    w = flat[off:off + 200].astype(np.float64)
    assert 0.5 * (2.0 / 25) < w.var() < 1.6 * (2.0 / 25)  # fan-in k*k = 25, not Ci*k*k
    fl = stacks.train_flops_per_image(SPEC, 33, 29)
    assert fl == 3.0 * (2.0 * 8 * 17 * 15 * 3 * 9 + 2.0 * 8 * 9 * 8 * 25 + 2.0 * 8 * 9 * 8 * 3)


def test_layer_names_count_dwconv_with_the_convolutions():
    from cnn_amd import hostapi

    assert hostapi._layer_names(SPEC)[:4] == ["conv_layer_1", "relu_layer_1", "dw_layer_2", "relu_layer_2"]
    assert hostapi._layer_names(stacks.resnet18())[:4] == ["conv_layer_1", "bn_layer_1", "relu_layer_1", "max_pool_1"]


def test_mobilenet_v1_walks_to_1024_in_front_of_the_head():
    spec = stacks.mobilenet_v1()
    layout = stacks.walk(spec, 3, 224, 224)
    assert "mobilenet_v1" not in stacks.STACKS and "mobilenet_v1" not in stacks.DEFAULT_BATCH
    assert layout[0]["kind"] == "conv" and layout[0]["out"] == (32, 112, 112)
    dws = [e for e in layout if e["kind"] == "dwconv"]
    assert len(dws) == 13 and all(e["k"] == 3 and e["pad"] == 1 for e in dws)
    assert [(e["in"][0], e["in"][1], e["s"]) for e in dws] == [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1),
                                                                (256, 28, 2)] + [(512, 14, 1)] * 5 + [(512, 14, 2), (1024, 7, 1)]
    assert sum(1 for e in layout if e["kind"] == "conv" and e["k"] == 1) == 13
    assert layout[-2]["kind"] == "pool" and layout[-2]["in"] == (1024, 7, 7) and layout[-2]["out"] == (1024, 1, 1)
    assert layout[-1]["kind"] == "linear" and layout[-1]["n_in"] == 1024 and layout[-1]["n_out"] == 3
    assert sum(1 for e in layout if e["kind"] == "bn") == 27 and sum(1 for e in stacks.walk(stacks.mobilenet_v1(batch_norm=False)) if e["kind"] == "bn") == 0
