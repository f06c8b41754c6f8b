"""Stream order of the layer, loss-head and device-helper entry points, caller late through the capi wrappers (tests/stream_order.py is
the harness; tests/stream_order_cases.py holds the inputs and the CPU references): max-pool, ReLU, Dropout, linear, BatchNorm2d in
every form, the five sync-BN phase entry points, the hard and soft loss heads, cnn_loss_from_terms, cnn_soft_targets, cnn_batch_mix,
cnn_eval_accumulate / cnn_eval_read, cnn_grad_cam and cnn_augment_u8."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_order as SO
from tests import stream_order_cases as K
from tests.util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture
def H(T):
    h = SO.harness(T)
    try:
        yield h
    finally:
        h.finish()


def _runner(T, name, t):
    """-> (call() -> {output: tensor} run with S current, [workspaces to poison]) of one case on its late operands t"""
    from cnn_amd import capi

    lib, P, S = capi.load(), capi._ptr, capi._stream
    f7 = lambda shape: T.full(tuple(shape), 7.0, dtype=T.float32, device="cuda")
    i7 = lambda shape: T.full(tuple(shape), 7, dtype=T.int32, device="cuda")
    poison = []
    if name == "maxpool_forward":
        def call():
            y, mask = f7((2, 3, 4, 5)), i7((2, 3, 4, 5))
            capi.check(lib.cnn_maxpool2d_forward(P(t["x"]), P(y), P(mask), *K.POOL_SHAPE, 3, 2, S()), name)
            return {"y": y, "mask": mask}
    elif name == "maxpool_backward":
        call = lambda: {"dx": capi.maxpool_backward(t["dy"], t["mask"], K.POOL_SHAPE, 3, 2, dx=f7(K.POOL_SHAPE))}
    elif name == "maxpool_backward_relu":
        call = lambda: {"dx": capi.maxpool_backward_relu(t["dy"], t["mask"], t["pooled"], K.POOL_SHAPE, 3, 2, dx=f7(K.POOL_SHAPE))}
    elif name == "relu_forward":
        call = lambda: {"y": capi.relu_forward(t["x"], f7(t["x"].shape))}
    elif name == "relu_backward":
        call = lambda: {"dy": capi.relu_backward(t["y"], t["dy"])}
    elif name.startswith("dropout_forward"):
        call = lambda: {"y": capi.dropout_forward(t["x"], 0.5, name.endswith("train"), f7(t["x"].shape))}
    elif name == "dropout_backward":
        call = lambda: {"dy": capi.dropout_backward(t["dy"], 0.5)}
    elif name == "linear_forward":
        call = lambda: {"y": capi.linear_forward(t["x"], t["w"], t["bias"], f7((K.LIN[0], K.LIN[2])))}
    elif name.startswith("linear_backward"):
        def call():
            gw, gb, dx = f7(t["w"].shape), f7((K.LIN[2],)), f7(t["x"].shape)
            capi.linear_backward(t["x"], t["dy"], t["w"], float(K.LIN[0]), gw, gb, dx, relu_below=name.endswith("relu"))
            return {"gw": gw, "gb": gb, "dx": dx}
    elif name.startswith(("batchnorm_", "syncbn_")):
        shape = tuple(t["x"].shape) if "x" in t else K.BN_POOLED
        bn = capi.BatchNorm2d(*shape)
        poison = [bn.ws]
        same = lambda s: None  # the all-reduce of one process
        count = shape[0] * shape[2] * shape[3]
        if "forward" in name:
            training, relu = "_eval" not in name, "_relu" in name

            def call():
                bn.saved_mean.fill_(7.0)
                bn.saved_var.fill_(7.0)
                out = {"moving_mean": t["moving_mean"], "moving_var": t["moving_var"]}
                args = (t["x"], t["gamma"], t["beta"], t["moving_mean"], t["moving_var"])
                if name == "batchnorm_forward_relu_pool":
                    B, Cc, Hh, Ww = shape
                    out["pooled"], mask, y_relu = f7((B, Cc, Hh // 2, Ww // 2)), i7((B, Cc, Hh // 2, Ww // 2)), f7(shape)
                    bn.forward_relu_pool(*args, out["pooled"], mask, y_relu=y_relu)
                    out["pooled_by_mask"] = T.gather(y_relu.view(B, -1), 1, mask.view(B, -1).long()).view(out["pooled"].shape)
                else:
                    out["y"] = f7(shape)
                    if relu:
                        out["y_relu"] = f7(shape)
                    if name.startswith("syncbn"):
                        bn.forward_sync(*args, out["y"], same, count, y_relu=out.get("y_relu"))
                    else:
                        bn.forward(*args, out["y"], training=training, y_relu=out.get("y_relu"))
                if training:
                    out.update(saved_mean=bn.saved_mean, saved_var=bn.saved_var)
                return out
        else:
            def call():
                bn.saved_mean.copy_(t["saved_mean"])  # (on S, behind the late operands: the layer object owns its statistics)
                bn.saved_var.copy_(t["saved_var"])
                gg, gb = f7((shape[1],)), f7((shape[1],))
                if name == "batchnorm_backward_pooled":
                    dx = bn.backward_pooled(t["x"], t["dpool"], t["mask"], t["pooled"], t["gamma"], gg, gb, f7(shape))
                elif name.startswith("syncbn"):
                    dx = bn.backward_sync(t["x"], t["dy"], t["gamma"], gg, gb, same, count)
                else:
                    dx = bn.backward(t["x"], t["dy"], t["gamma"], gg, gb)
                return {"dx": dx, "ggamma": gg, "gbeta": gb}
    elif name.startswith("softmax_xent"):
        def call():
            fn = capi.softmax_xent_soft if "targets" in t else capi.softmax_xent
            probs, delta, loss = fn(t["logits"], t["targets"] if "targets" in t else t["labels"])
            return {"probs": probs, "delta": delta, "loss_sum": loss}
    elif name.startswith("linear_softmax_xent"):
        def call():
            B, n_in, soft, dx = K.HEAD_B, K.HEAD_IN, "targets" in t, name.endswith("_dx")
            out = {"logits": f7((B, 3)), "probs": f7((B, 3)), "delta": f7((B, 3)), "loss_terms": f7((B,))}
            head = [P(t["x"]), P(t["w"]), P(t["bias"]), P(t["targets"] if soft else t["labels"])] + [P(out[k]) for k in ("logits", "probs", "delta", "loss_terms")]
            fn = getattr(lib, "cnn_linear_forward_softmax_xent" + ("_soft" if soft else "") + ("_dx" if dx else ""))
            if dx:
                out["dx"] = f7((B, n_in))
                capi.check(fn(*head, P(out["dx"]), 1, B, n_in, 3, S()), name)
            else:
                capi.check(fn(*head, B, n_in, 3, S()), name)
            return out
    elif name == "loss_from_terms":
        def call():
            loss = f7((1,))
            capi.check(lib.cnn_loss_from_terms(P(t["loss_terms"]), P(loss), K.HEAD_B, S()), name)
            return {"loss_sum": loss}
    elif name == "soft_targets":
        call = lambda: {"targets": capi.soft_targets(t["labels"], 10, 0.1, 0.7, capi.PAIR_ROLL, 1, out=f7((K.HEAD_B, 10)))}
    elif name.startswith("batch_mix"):
        mix = capi.MixDesc(capi.MIX_MIXUP, 0.3, capi.PAIR_FLIP, 0, 0, 0, 0, 0) if name.endswith("mixup") else \
            capi.MixDesc(capi.MIX_CUTMIX, 1.0, capi.PAIR_ROLL, 1, 2, 7, 1, 6)
        call = lambda: {"dst": capi.batch_mix(mix, t["src"], f7(t["src"].shape))}
    elif name == "eval_accumulate":
        def call():
            state = T.full((capi.eval_state_bytes(10),), 7, dtype=T.uint8, device="cuda")
            capi.check(lib.cnn_memset_zero(P(state), state.numel(), S()), "cnn_memset_zero")
            pred = capi.eval_accumulate(t["logits"], t["labels"], state, k=3, pred=i7((K.HEAD_B,)))
            return {"pred": pred, "counts_and_confusion": T.cat([state[:32], state[40:]]), "loss_sum": state[32:40].clone().view(T.float64)}
    elif name == "eval_read":
        def call():
            got = capi.eval_read(t["state"], 10)
            host = lambda a: T.from_numpy(np.asarray(a, np.float64).reshape(-1)).cuda()
            return {"counts": host([got["samples"], got["top1"], got["topk"], got["ignored"]]), "loss_sum": host([got["loss_sum"]]),
                    "confusion": host(got["confusion"])}
    elif name == "grad_cam":
        def call():
            cam, img = capi.grad_cam(t["feature"])
            return {"cam": cam, "image": img}
    else:
        assert name == "augment_u8"
        call = lambda: {"out": capi.augment_u8(t["src"], t["matrices"], 8, 8, fill=0.25, out=f7((2, 3, 8, 8)))}
    return call, poison


@pytest.mark.parametrize("name", sorted(K.LAYERS))
def test_layer_calls_caller_late(T, H, name):
    """the operands arrive late on S, outputs hold 7.0, workspaces a poison: the clones behind the call equal the CPU reference --
    bit for bit where tests/stream_order_cases.py::EXACT names the output, to REL_TOL (tensor-normalised) otherwise"""
    inputs, reference = K.LAYERS[name]
    inp, decoys = inputs(), K.layer_decoys(name)
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {n: dev(a) for n, a in inp.items()}
    T.cuda.synchronize()
    late = [H.late(t[n], 0, decoy=dev(decoys[n])) for n in sorted(t)]
    call, poison = _runner(T, name, t)
    res = H.caller_late("layer " + name, late, call, poison=poison, blocks=name in K.LAYER_BLOCKS)
    ref = reference(inp)
    assert not isinstance(res.gated, int) and sorted(res.gated) == sorted(ref), (name, res.gated)
    for out, want in ref.items():
        got = res.gated[out]
        if out in K.EXACT.get(name, ()):
            assert got.shape == np.asarray(want).shape, (name, out)
            assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).astype(got.dtype).tobytes(), f"{name}: {out} differs"
        elif out == "image":  # (8-bit picture of a plane held to REL_TOL: one step of the byte)
            assert np.abs(got.astype(np.int32).reshape(want.shape) - want.astype(np.int32)).max() <= 1, name
        else:
            assert_close(got.reshape(np.asarray(want).shape), want, REL_TOL, f"stream order, {name}: {out}")
    res.assert_same_bits_as_plain(name)
