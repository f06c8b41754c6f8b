"""Inputs, decoys and CPU references of the stream-order cases that are not held by a recorded digest (tests/stream_order.py is the
harness).  Needs no device: tests/test_stream_order_decoys.py checks here that no decoy gives the real answer."""
import numpy as np

from tests.stream_order import decoy_of
from tests.util import normal_scaled, uniform01, uniform_pm1

# ---- fork and join: cnn_conv2d_backward*, cnn_conv2d_backward_weight_side, cnn_amd_side_stream_join, cnn_amd_flush_reduces ----------
FORK_DESCS = [
    (2, 16, 55, 55, 32, 3, 2, 0),
    (2, 32, 14, 14, 64, 3, 1, 1),
    (2, 3, 56, 56, 16, 3, 2, 0),
    (2, 5, 13, 11, 7, 5, 2, 0),   # reaches the split-K slabs and their reduction
]
POOLED_DESC = FORK_DESCS[2]       # the one desc of the four that the pool-fused first block covers
# variant -> the inputs it reads
FORK_VARIANTS = {
    "backward_join_now": ("x", "dy", "w"),                  # cnn_conv2d_backward, defer_join = 0
    "backward_deferred_join": ("x", "dy", "w"),             # defer_join = 1, then cnn_amd_side_stream_join
    "backward_deferred_flush_join": ("x", "dy", "w"),       # defer_join = 1, cnn_amd_flush_reduces on the side stream, then the join
    "weight_side_join": ("x", "dy"),                        # cnn_conv2d_backward_weight_side, then the join
    "prepared_join_now": ("x", "dy", "pd"),                 # cnn_conv2d_backward_prepared, defer_join = 0
    "prepared_deferred_join": ("x", "dy", "pd"),
    "prepared_relu_join_now": ("x", "dy", "pd", "relu_below"),   # cnn_conv2d_backward_prepared_relu
    "prepared_relu_deferred_join": ("x", "dy", "pd", "relu_below"),
    "pooled2_join_now": ("x", "dpool", "mask", "pooled", "pd"),  # cnn_conv2d_backward_pooled2_prepared
    "pooled2_deferred_join": ("x", "dpool", "mask", "pooled", "pd"),
}


def fork_cases():
    return [(d, v) for d in FORK_DESCS for v in FORK_VARIANTS if not v.startswith("pooled2") or d == POOLED_DESC]


def fork_seed(case):
    return 7100 + 10 * FORK_DESCS.index(case)


def fork_inputs(case, decoy=False):
    """{name: numpy} of one desc: x, w, dy, relu_below and, for POOLED_DESC, the pooled-domain operands (pooled and mask are the
    ORACLE's forward results: inputs of the call like any other).  decoy: the same names from another seed"""
    from oracle import pyoracle as O

    B, Ci, H, W, Co, k, s, pad = case
    seed = fork_seed(case)
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    x = uniform01(seed, (B, Ci, H, W))
    inp = {"x": x, "w": normal_scaled(seed + 1, (Co, Ci, k, k)), "dy": uniform_pm1(seed + 3, (B, Co, Ho, Wo)),
           "relu_below": np.where(x - np.float32(0.5) >= 0, x - np.float32(0.5), np.float32(0)).astype(np.float32)}
    if case == POOLED_DESC:
        bias = normal_scaled(seed + 2, (Co,))
        relu = O.relu_forward(O.conv2d_forward_padded(x, inp["w"], bias, s, pad))
        pooled, mask = O.maxpool_forward(relu, 2, 2)
        inp.update(bias=bias, pooled=pooled, mask=mask, dpool=uniform_pm1(seed + 4, pooled.shape))
    if decoy:
        return {name: decoy_of(a, seed + 50 + i) for i, (name, a) in enumerate(sorted(inp.items()))}
    return inp


def fork_reference(case, variant, inp):
    """{gw, gb, dx} (weight_side: no dx) of the CPU oracle"""
    from oracle import pyoracle as O

    B, Ci, H, W, Co, k, s, pad = case
    if variant.startswith("pooled2"):
        shape = (B, Co, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1)
        # MaxPool2D::backward of dpool, then ReLU::backward by the pooled value at the window's maximum -- stated from the call's
        # operands alone, so that it also says what the call makes of a decoy
        dy = O.maxpool_backward(inp["dpool"], inp["mask"], shape, 2, 2)
        open_ = O.maxpool_backward((inp["pooled"] > 0).astype(np.float32), inp["mask"], shape, 2, 2)
        dy = np.where(open_ > 0, dy, np.float32(0)).astype(np.float32)
    else:
        dy = inp["dy"]
    gw, gb, dx = O.conv2d_backward_padded(inp["x"], dy, inp["w"], s, pad)
    if variant.startswith("prepared_relu"):
        dx = np.where(inp["relu_below"] <= 0, np.float32(0), dx)
    out = {"gw": gw, "gb": gb, "dx": dx}
    if variant == "weight_side_join":
        del out["dx"]
    return out


# ---- published kernels -------------------------------------------------------------------------------------------------------------
def published_linear_inputs(decoy=False):
    """linear backward, B = 4, 64 -> 3 (a launch_pub site)"""
    inp = {"x": uniform_pm1(7301, (4, 64)),"dy": uniform_pm1(7302, (4, 3)), "w": normal_scaled(7303, (64, 3))}
    return {n: decoy_of(a, 7350 + i) for i, (n, a) in enumerate(sorted(inp.items()))} if decoy else inp


def published_linear_reference(inp):
    from oracle import pyoracle as O

    gw, gb, dx = O.linear_backward(inp["x"], inp["dy"], inp["w"])
    return {"gw": gw, "gb": gb, "dx": np.where(inp["x"] <= 0, np.float32(0), dx)}


def published_relu_inputs(decoy=False):
    inp = {"x": uniform_pm1(7311, (1027,))}
    return {"x": decoy_of(inp["x"], 7360)} if decoy else inp


def published_relu_reference(inp):
    return {"y": np.where(inp["x"] >= 0, inp["x"], np.float32(0)).astype(np.float32)}


# ---- layers, loss heads and the small device helpers: name -> (inputs() -> {name: numpy}, reference(inputs) -> {name: numpy}) -------
# An output named in EXACT is held bit for bit (selections, copies and rules the project restates in NumPy bit for bit); every other one
# to REL_TOL, tensor-normalised, against the CPU oracle.
F = np.float32
POOL_SHAPE, LIN, BN_POOLED = (2, 3, 9, 11), (3, 50, 7), (6, 5, 60, 52)
HEAD_B, HEAD_IN = 5, 50


def _pool_fwd(seed):
    from oracle import pyoracle as O

    x = uniform_pm1(seed, POOL_SHAPE)
    y, mask = O.maxpool_forward(x, 3, 2)
    return x, y, mask


def _open_windows(dpool, mask, pooled, shape, k, step):
    """MaxPool2D::backward followed by the ReLU::backward that tests the pooled value, from the call's operands alone"""
    from oracle import pyoracle as O

    d = O.maxpool_backward(dpool, mask, shape, k, step)
    open_ = O.maxpool_backward((np.asarray(pooled) > 0).astype(F), mask, shape, k, step)
    return np.where(open_ > 0, d, F(0)).astype(F)


def _bn_inputs(shape, seed):
    C = shape[1]
    return {"x": uniform_pm1(seed, shape), "gamma": uniform01(seed + 1, (C,)) + F(0.5), "beta": uniform_pm1(seed + 2, (C,)),
            "moving_mean": uniform_pm1(seed + 3, (C,)), "moving_var": uniform01(seed + 4, (C,)) + F(0.5)}


def _bn_forward_ref(inp, training, relu):
    from oracle import pyoracle as O

    y, _, sm, sv, mm, mv = O.batchnorm_forward(inp["x"], inp["gamma"], inp["beta"], inp["moving_mean"], inp["moving_var"], training=training)
    out = {"y": y, "moving_mean": mm, "moving_var": mv}
    if training:
        out.update(saved_mean=sm, saved_var=sv)
    if relu:
        out["y_relu"] = np.where(y >= 0, y, F(0)).astype(F)
    return out


def _bn_backward_inputs(shape, seed):
    from oracle import pyoracle as O

    inp = _bn_inputs(shape, seed)
    _, _, sm, sv, _, _ = O.batchnorm_forward(inp["x"], inp["gamma"], inp["beta"], inp["moving_mean"], inp["moving_var"], training=True)
    return {"x": inp["x"], "dy": uniform_pm1(seed + 5, shape), "gamma": inp["gamma"], "saved_mean": sm, "saved_var": sv}


def _bn_backward_ref(inp):
    from oracle import pyoracle as O

    dx, gg, gb = O.batchnorm_backward(inp["x"], inp["dy"], inp["gamma"], inp["saved_mean"], inp["saved_var"])
    return {"dx": dx, "ggamma": gg, "gbeta": gb}


def _bn_pooled_forward_ref(inp):
    from oracle import pyoracle as O

    out = _bn_forward_ref(inp, True, True)
    pooled, _ = O.maxpool_forward(out["y_relu"], 2, 2)
    # (the mask is held through pooled_by_mask: what the ReLU output holds where the call's mask points; an index comparison would
    # count a tie between two pixels that differ in the last bit as a failure)
    return {"pooled": pooled, "pooled_by_mask": pooled, "saved_mean": out["saved_mean"], "saved_var": out["saved_var"],
            "moving_mean": out["moving_mean"], "moving_var": out["moving_var"]}


def _bn_pooled_backward_inputs():
    from oracle import pyoracle as O

    inp = _bn_inputs(BN_POOLED, 7530)
    fwd = _bn_forward_ref(inp, True, True)
    pooled, mask = O.maxpool_forward(fwd["y_relu"], 2, 2)
    return {"x": inp["x"], "dpool": uniform_pm1(7536, pooled.shape), "mask": mask, "pooled": pooled, "gamma": inp["gamma"],
            "saved_mean": fwd["saved_mean"], "saved_var": fwd["saved_var"]}


def _bn_pooled_backward_ref(inp):
    dy = _open_windows(inp["dpool"], inp["mask"], inp["pooled"], BN_POOLED, 2, 2)
    return _bn_backward_ref(dict(inp, dy=dy))


def _head_inputs(classes, soft, fused):
    labels = ((np.arange(HEAD_B) * 2 + 1) % classes).astype(np.int32)
    inp = {}
    if fused:
        inp.update(x=uniform_pm1(7540, (HEAD_B, HEAD_IN)), w=normal_scaled(7541, (HEAD_IN, classes), 0.3), bias=normal_scaled(7542, (classes,)))
    else:
        inp["logits"] = uniform_pm1(7543 + classes, (HEAD_B, classes)) * F(3)
    if soft:
        from tests.soft_target_ref import PAIR_ROLL, ref_soft_targets

        inp["targets"] = ref_soft_targets(labels, classes, 0.1, 0.7, PAIR_ROLL, 1)
    else:
        inp["labels"] = labels
    return inp


def _head_ref(inp, dx, relu_below=True):
    """float64 softmax / cross-entropy of the (oracle's) logits: probs, delta, loss terms, loss sum and, for the fused heads, logits / dx"""
    from oracle import pyoracle as O

    out = {}
    if "x" in inp:
        logits = O.linear_forward(inp["x"], inp["w"], inp["bias"])
        out["logits"] = logits
    else:
        logits = inp["logits"]
    classes = logits.shape[1]
    t = inp["targets"].astype(np.float64) if "targets" in inp else (inp["labels"][:, None] == np.arange(classes)[None, :]).astype(np.float64)
    z = logits.astype(np.float64) - logits.astype(np.float64).max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    out["probs"], out["delta"] = np.exp(logp).astype(F), (np.exp(logp) - t).astype(F)
    terms = (t * logp).sum(axis=1)
    if "x" in inp:
        out["loss_terms"] = terms.astype(F)
        if dx:
            d = O.linear_backward(inp["x"], out["delta"], inp["w"])[2]
            out["dx"] = np.where(inp["x"] <= 0, F(0), d).astype(F) if relu_below else d
    else:
        out["loss_sum"] = np.array([-terms.sum()], F)
    return out


def _eval_inputs():
    labels = np.array([1, 9, -1, 3, 0], np.int32)   # one ignored sample (a padded batch)
    return {"logits": uniform_pm1(7560, (HEAD_B, 10)) * F(3), "labels": labels}


def eval_state_of(total):
    """the bytes of the device's evaluation state block (include/cnn_amd.h) for the totals of tests/eval_ref.py"""
    head = np.array([total["samples"], total["top1"], total["topk"], total["ignored"]], np.uint64).tobytes()
    return np.frombuffer(head + np.float64(total["loss_sum"]).tobytes() + np.ascontiguousarray(total["confusion"], np.uint64).tobytes(), np.uint8).copy()


def _eval_ref(inp):
    from tests.eval_ref import ref_accumulate, ref_batch

    one = ref_batch(inp["logits"], inp["labels"], 3)
    state = eval_state_of(ref_accumulate([one]))
    # the integers of the state block bit for bit; the loss sum to REL_TOL (its terms go through the device's logf / expf)
    return {"pred": one["pred"], "counts_and_confusion": np.concatenate([state[:32], state[40:]]), "loss_sum": np.frombuffer(state[32:40].tobytes(), np.float64).copy()}


def _eval_read_inputs():
    from tests.eval_ref import ref_accumulate, ref_batch

    inp = _eval_inputs()
    return {"state": eval_state_of(ref_accumulate([ref_batch(inp["logits"], inp["labels"], 3)] * 2))}


def _eval_read_ref(inp):
    s = inp["state"]
    counts = np.frombuffer(s[:32].tobytes(), np.uint64).astype(np.float64)
    return {"counts": counts, "loss_sum": np.frombuffer(s[32:40].tobytes(), np.float64).copy(),
            "confusion": np.frombuffer(s[40:].tobytes(), np.uint64).astype(np.float64)}


def _augment_inputs():
    src = np.random.RandomState(7570).randint(0, 256, size=(2, 9, 11, 3)).astype(np.uint8)
    # sample 0: the plain 9 x 11 -> 8 x 8 resize map (half-pixel centres); sample 1: mirrored and turned by 30 degrees about the centre
    sx, sy = 11 / 8, 9 / 8
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    m = np.array([[sx, 0, 0.5 * sx - 0.5, 0, sy, 0.5 * sy - 0.5],
                  [-c * sx, s * sy, 9.0, s * sx, c * sy, 0.5]], F)
    return {"src": src, "matrices": m}


def _augment_ref(inp):
    from tests.augment_ref import augment

    return {"out": augment(inp["src"], inp["matrices"], 8, 8, fill=0.25)[0]}


def _grad_cam_ref(inp):
    from oracle import pyoracle as O

    cam, img = O.grad_cam(inp["feature"])
    return {"cam": cam, "image": img}


def _mix_ref(inp, mode):
    from tests.soft_target_ref import MIX_CUTMIX, MIX_MIXUP, PAIR_FLIP, PAIR_ROLL, ref_batch_mix

    if mode == "mixup":
        return {"dst": ref_batch_mix(inp["src"], MIX_MIXUP, 0.3, PAIR_FLIP)}
    return {"dst": ref_batch_mix(inp["src"], MIX_CUTMIX, 1.0, PAIR_ROLL, 1, (2, 7, 1, 6))}


def _layers():
    from oracle import pyoracle as O
    from tests.soft_target_ref import PAIR_ROLL, ref_soft_targets

    L = {}
    L["maxpool_forward"] = (lambda: {"x": _pool_fwd(7500)[0]}, lambda i: dict(zip(("y", "mask"), O.maxpool_forward(i["x"], 3, 2))))
    L["maxpool_backward"] = (lambda: {"dy": uniform_pm1(7501, _pool_fwd(7500)[1].shape), "mask": _pool_fwd(7500)[2]},
                             lambda i: {"dx": O.maxpool_backward(i["dy"], i["mask"], POOL_SHAPE, 3, 2)})
    L["maxpool_backward_relu"] = (lambda: {"dy": uniform_pm1(7501, _pool_fwd(7500)[1].shape), "mask": _pool_fwd(7500)[2], "pooled": _pool_fwd(7500)[1]},
                                  lambda i: {"dx": O.maxpool_backward(np.where(i["pooled"] <= 0, F(0), i["dy"]).astype(F), i["mask"], POOL_SHAPE, 3, 2)})
    L["relu_forward"] = (lambda: {"x": uniform_pm1(7502, (1027,))}, lambda i: {"y": np.where(i["x"] >= 0, i["x"], F(0)).astype(F)})
    L["relu_backward"] = (lambda: {"y": np.maximum(uniform_pm1(7503, (1027,)), 0), "dy": uniform_pm1(7504, (1027,))},
                          lambda i: {"dy": np.where(i["y"] <= 0, F(0), i["dy"]).astype(F)})
    for training in (True, False):
        L[f"dropout_forward_{'train' if training else 'eval'}"] = (lambda: {"x": uniform_pm1(7505, (2, 4, 3, 5))},
                                                                   lambda i, t=training: {"y": O.dropout_forward(i["x"], 0.5, t)})
    L["dropout_backward"] = (lambda: {"dy": uniform_pm1(7506, (2, 4, 3, 5))}, lambda i: {"dy": O.dropout_backward(i["dy"], 0.5)})
    B, n_in, n_out = LIN
    lin = lambda: {"x": uniform_pm1(7510, (B, n_in)), "w": normal_scaled(7511, (n_in, n_out)), "bias": normal_scaled(7512, (n_out,)),
                   "dy": uniform_pm1(7513, (B, n_out))}
    L["linear_forward"] = (lambda: {k: v for k, v in lin().items() if k != "dy"}, lambda i: {"y": O.linear_forward(i["x"], i["w"], i["bias"])})
    for relu in (False, True):
        def lin_bwd(i, relu=relu):
            gw, gb, dx = O.linear_backward(i["x"], i["dy"], i["w"])
            return {"gw": gw, "gb": gb, "dx": np.where(i["x"] <= 0, F(0), dx).astype(F) if relu else dx}
        L["linear_backward" + ("_relu" if relu else "")] = (lambda: {k: v for k, v in lin().items() if k != "bias"}, lin_bwd)
    for shape in ((2, 4, 8, 8), (2, 32, 8, 8)):
        tag = "x".join(str(v) for v in shape)
        for training, relu in ((True, False), (False, False), (True, True), (False, True)):
            name = f"batchnorm_forward{'_relu' if relu else ''}_{'train' if training else 'eval'}_{tag}"
            L[name] = (lambda s=shape: _bn_inputs(s, 7520), lambda i, t=training, r=relu: _bn_forward_ref(i, t, r))
        L[f"batchnorm_backward_{tag}"] = (lambda s=shape: _bn_backward_inputs(s, 7520), _bn_backward_ref)
    L["batchnorm_forward_relu_pool"] = (lambda: _bn_inputs(BN_POOLED, 7530), _bn_pooled_forward_ref)
    L["batchnorm_backward_pooled"] = (_bn_pooled_backward_inputs, _bn_pooled_backward_ref)
    # sync-BN with one process: partial_sums (twice), forward_from_sums[_relu], backward_sums, backward_from_sums
    L["syncbn_forward"] = (lambda: _bn_inputs((2, 4, 8, 8), 7520), lambda i: _bn_forward_ref(i, True, False))
    L["syncbn_forward_relu"] = (lambda: _bn_inputs((2, 4, 8, 8), 7520), lambda i: _bn_forward_ref(i, True, True))
    L["syncbn_backward"] = (lambda: _bn_backward_inputs((2, 4, 8, 8), 7520), _bn_backward_ref)
    for classes in (3, 10):
        for soft in (False, True):
            L[f"softmax_xent{'_soft' if soft else ''}_{classes}"] = (lambda c=classes, s=soft: _head_inputs(c, s, False), lambda i: _head_ref(i, False))
    for soft in (False, True):
        for dx in (False, True):
            L[f"linear_softmax_xent{'_soft' if soft else ''}{'_dx' if dx else ''}"] = (lambda s=soft: _head_inputs(3, s, True),
                                                                                      lambda i, d=dx: _head_ref(i, d))
    L["loss_from_terms"] = (lambda: {"loss_terms": -uniform01(7550, (HEAD_B,)) - F(0.1)},
                            lambda i: {"loss_sum": np.array([-i["loss_terms"].astype(np.float64).sum()], F)})
    L["soft_targets"] = (lambda: {"labels": np.array([1, 9, 4, 3, 0], np.int32)},
                         lambda i: {"targets": ref_soft_targets(i["labels"], 10, 0.1, 0.7, PAIR_ROLL, 1)})
    for mode in ("mixup", "cutmix"):
        L[f"batch_mix_{mode}"] = (lambda: {"src": uniform_pm1(7555, (4, 3, 8, 8))}, lambda i, m=mode: _mix_ref(i, m))
    L["eval_accumulate"] = (_eval_inputs, _eval_ref)
    L["eval_read"] = (_eval_read_inputs, _eval_read_ref)
    L["grad_cam"] = (lambda: {"feature": uniform_pm1(7565, (2, 4, 6, 6))}, _grad_cam_ref)
    L["augment_u8"] = (_augment_inputs, _augment_ref)
    return L


LAYERS = _layers()
EXACT = {"maxpool_forward": {"y", "mask"}, "maxpool_backward": {"dx"}, "maxpool_backward_relu": {"dx"}, "relu_forward": {"y"},
         "relu_backward": {"dy"}, "dropout_forward_train": {"y"}, "dropout_backward": {"dy"}, "soft_targets": {"targets"},
         "batch_mix_mixup": {"dst"}, "batch_mix_cutmix": {"dst"}, "eval_accumulate": {"pred", "counts_and_confusion"}, "eval_read": {"counts", "loss_sum", "confusion"},
         "augment_u8": {"out"}}
# calls that wait for the device by contract
LAYER_BLOCKS = {"eval_read"}


def layer_decoys(name):
    """the decoys of one case: another seed's data, valid for the call (a variance stays positive)"""
    inp = LAYERS[name][0]()
    out = {n: decoy_of(a, 7700 + 7 * i + sum(map(ord, name)) % 97) for i, (n, a) in enumerate(sorted(inp.items()))}
    for n in out:
        if n.endswith("_var"):
            out[n] = np.abs(out[n]) + F(0.25)
    return out


# ---- the first block outside the fork / join family, the im2col fallback, the tile measurement ---------------------------------------
IM2COL_DESC = FORK_DESCS[3]
TUNE_SHAPE = (2, 10, 12, 12, 5, 1, 2)     # B, Ci, H, W, k, s, pad of the measured geometries: 5x5, served by the implicit GEMM only
TUNE_CO = (20, 24, 28, 32, 36, 40)        # one Co per call: a geometry is measured once per process, so every run needs a fresh one


def first_block_forward_reference(inp):
    """POOLED_DESC through Conv2D -> ReLU -> MaxPool2D(2, 2): the pooled tensor and the ReLU output the mask is checked against"""
    from oracle import pyoracle as O

    relu = O.relu_forward(O.conv2d_forward_padded(inp["x"], inp["w"], inp["bias"], POOLED_DESC[6], POOLED_DESC[7]))
    return {"pooled": O.maxpool_forward(relu, 2, 2)[0], "relu": relu}


def pooled_by_mask(relu, mask):
    """what the ReLU output holds where an int32 pool mask (bit 31 = "pooled value <= 0" cleared) points"""
    B = relu.shape[0]
    idx = (np.asarray(mask).astype(np.int64) & 0x7FFFFFFF).reshape(B, -1)
    return np.take_along_axis(relu.reshape(B, -1), idx, 1).reshape(mask.shape)


def im2col_reference(inp):
    from oracle import pyoracle as O

    B, Ci, H, W, Co, k, s, pad = IM2COL_DESC
    gw, gb, dx = O.conv2d_backward_padded(inp["x"], inp["dy"], inp["w"], s, pad)
    return {"y": O.conv2d_forward_padded(inp["x"], inp["w"], inp["bias"], s, pad), "gw": gw, "gb": gb, "dx": dx}


def im2col_inputs(decoy=False):
    B, Ci, H, W, Co, k, s, pad = IM2COL_DESC
    inp = dict(fork_inputs(IM2COL_DESC), bias=normal_scaled(7390, (Co,)))
    return {n: decoy_of(a, 7395 + i) for i, (n, a) in enumerate(sorted(inp.items()))} if decoy else inp


def tune_inputs(decoy=False):
    B, Ci, H, W, k, s, pad = TUNE_SHAPE
    inp = {"x": uniform01(7380, (B, Ci, H, W)), "w": normal_scaled(7381, (max(TUNE_CO), Ci, k, k)), "bias": normal_scaled(7382, (max(TUNE_CO),))}
    return {n: decoy_of(a, 7385 + i) for i, (n, a) in enumerate(sorted(inp.items()))} if decoy else inp


def tune_reference(inp, co):
    from oracle import pyoracle as O

    return {"y": O.conv2d_forward_padded(inp["x"], inp["w"][:co], inp["bias"][:co], TUNE_SHAPE[5], TUNE_SHAPE[6])}
