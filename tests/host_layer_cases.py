"""Call sequences through the C++ host layers (cnn_amd/host: layers.cpp, sequential.cpp) and the record behind
tests/golden/host_layer_traces.json.

The maker (tests/golden/make_host_layer_traces.py) and the test (test_gpu_host_layer_traces.py) call the SAME function here.  A case is a
net and a sequence of calls, not a shape: what it pins is which kernels the layers launch for that sequence ("<kernel>|<geometry>" ->
launches) and the bytes they leave behind (SHA-256 of parameters, gradients, every layer's output, the input delta where it is valid,
the loss).  The file was recorded with the host library of the commit BEFORE the layer classes were rebuilt from shared parts and
must keep passing across host-side refactors; profiles/host_layers.md lists which branch of every forward / backward each case reaches."""
import hashlib
import re
import zlib

import numpy as np

from tests.util import uniform01

# ---- nets ------------------------------------------------------------------------------------------------------------------------
# the reference net at B = 4, 224 x 224 (the pool-fused first block exists only for that geometry)
# the small nets: 8 x 8 plane, B = 2.  C < 32 keeps BatchNorm2D off the channel-resident kernel, H even and W % 4 == 0 admit its pooled backward
def _bn(c):
    return [("conv", c, 3, 1, 1), ("bn",), ("relu",), ("pool", 2, 2), ("linear", 3)]


NETS = {
    "ref": (None, (3, 224, 224), 4),
    "bn8": (_bn(8), (3, 8, 8), 2),
    "bn32": (_bn(32), (3, 8, 8), 2),  # the channel-resident BatchNorm2D kernels
    "dropout": ([("conv", 8, 3, 1, 1), ("relu",), ("dropout", 0.5), ("pool", 2, 2), ("linear", 3)], (3, 8, 8), 2),
    "crcrl": ([("conv", 8, 3, 1, 1), ("relu",), ("conv", 8, 3, 1, 1), ("relu",), ("linear", 3)], (3, 8, 8), 2),
    # nets that END in a layer whose backward works in place: with host tensors (train_step_host) the loss delta is staged and written back
    "tail_relu": ([("conv", 3, 8, 1, 0), ("relu",)], (3, 8, 8), 2),
    "tail_bn": ([("conv", 3, 8, 1, 0), ("bn",)], (3, 8, 8), 2),
    "tail_dropout": ([("conv", 4, 8, 1, 0), ("dropout", 0.5)], (3, 8, 8), 2),
}

# ---- call sequences: ("step" [, B]) Sequential::train_step on a device batch; ("host_step",) the reference's loop on host tensors;
# ("fb",) Sequential::forward_backward; ("eval_host",) a no_grad forward of host tensors; ("set", switch, value); ("grad_cam", layer)
_TOGGLES = {
    "default": [("step",)] * 3,
    "fuse_pool_block=0": [("step",), ("set", "fuse_pool_block", 0), ("step",), ("step",)],
    "fuse_layers=0": [("step",), ("set", "fuse_layers", 0), ("step",), ("step",)],
    "input_gradient=0": [("step",), ("set", "input_gradient", 0), ("step",), ("step",)],
    "eval_then_step": [("step",), ("eval_host",), ("step",)],
    "partial_batch": [("step",), ("step",), ("step", -1), ("step",)],
    "host_steps": [("host_step",)] * 3,
}
CASES = {}
for _net in ("ref", "bn8", "bn32"):
    for _name, _ops in _TOGGLES.items():
        CASES[f"{_net}/{_name}"] = (_net, _ops)
CASES["ref/grad_cam"] = ("ref", [("step",), ("grad_cam", "conv_layer_1"), ("step",)])
CASES["bn8/grad_cam"] = ("bn8", [("step",), ("grad_cam", "bn_layer_1"), ("step",)])
CASES["bn8/forward_backward"] = ("bn8", [("step",), ("fb",), ("set", "fuse_layers", 0), ("fb",)])
for _net in ("dropout", "crcrl", "tail_relu", "tail_bn", "tail_dropout"):
    CASES[f"{_net}/host_steps"] = (_net, [("host_step",)] * 3)
for _net in ("dropout", "crcrl"):
    CASES[f"{_net}/default"] = (_net, _TOGGLES["default"])
    CASES[f"{_net}/fuse_layers=0"] = (_net, _TOGGLES["fuse_layers=0"])
# the linear layer's weight / bias gradient on a stream of its own (LinearLayer::backward after the loss head's data gradient; the one
# path on which Layer::join_pending has something to join): a third field names the library option the case runs under
for _net in ("ref", "bn8", "crcrl"):
    CASES[f"{_net}/linear_wb_own_stream"] = (_net, _TOGGLES["default"], ("LINEAR_WB_OWN_STREAM", 1))

SWITCHES = {"fuse_layers": "cnnh_set_fuse_layers", "fuse_pool_block": "cnnh_set_fuse_pool_block", "input_gradient": "cnnh_set_input_gradient"}


def build(net_name):
    """-> (net, layer names, walk() layout, input shape, batch)"""
    from cnn_amd import hostapi, stacks as S

    spec, in_shape, B = NETS[net_name]
    if spec is None:
        net = hostapi.HostAlexNet(3)
        spec = S.alexnet(3)
        return net, hostapi._layer_names(spec), S.walk(spec, *in_shape), in_shape, B
    net = hostapi.HostSequential(spec, in_shape)
    return net, net.names, net.layout, in_shape, B


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rc(error):
    """hostapi's exceptions name the C wrapper's return code (RuntimeError: code 3): -> "rc=<n>" """
    m = re.search(r"rc=(\d+)", str(error))
    return f"rc={m.group(1)}" if m else "rc=3"


def run_case(T, name, driver=None):
    """-> {"log": {key: launches}, "sha": {what: digest | "rc=<n>"}} of one case, on a fresh net and seeded inputs.
    driver (the stream-order tests; None leaves the run and its record as they are): driver.before_steps(xd, ld) is called with the
    device batch and labels in front of the call sequence, driver.before_op(i, op) / driver.after_op(i, op) around every call of it,
    driver.after_steps() behind the flush that follows it, before anything is read back; kernel timing then stays off and the log
    is empty"""
    from cnn_amd import capi, hostapi

    net_name, ops = CASES[name][:2]
    option = CASES[name][2] if len(CASES[name]) > 2 else None
    lib = hostapi.load()
    old_option = capi.get_option(option[0]) if option else None
    if option:
        capi.set_option(*option)
    net, names, layout, in_shape, B = build(net_name)
    seed = 7000 + zlib.crc32(name.encode()) % 1000
    x = uniform01(seed, (B,) + in_shape)
    labels = (np.arange(B) % 3).astype(np.int32)
    xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    sha, last_B, device_loss = {}, B, False
    T.cuda.synchronize()
    if driver is None:
        capi.kernel_timing(1)
    try:
        if driver is not None:
            driver.before_steps(xd, ld)
        for i, op in enumerate(ops):
            if driver is not None:
                driver.before_op(i, op)
            if op[0] == "step":
                last_B = B + op[1] if len(op) > 1 else B
                net.train_step(xd[:last_B], ld[:last_B], 1e-2)
                device_loss = True
            elif op[0] == "fb":
                net.forward_backward(xd, ld)
                last_B, device_loss = B, True
            elif op[0] == "host_step":
                loss, probs = net.train_step_host(x, labels, 1e-2)
                sha[f"{i}:host_loss"], sha[f"{i}:probs"], last_B = _sha(np.float32(loss)), _sha(probs), B
            elif op[0] == "eval_host":
                lib.cnnh_set_no_grad(1)
                try:
                    sha[f"{i}:logits"], last_B = _sha(net.forward_host(x)), B
                finally:
                    lib.cnnh_set_no_grad(0)
            elif op[0] == "set":
                getattr(lib, SWITCHES[op[1]])(op[2])
            elif op[0] == "grad_cam":
                C_, H_, W_ = layout[names.index(op[1])]["out"]
                img, cam = net.grad_cam(op[1], (last_B, H_, W_))
                sha[f"{i}:cam_image"], sha[f"{i}:cam"] = _sha(img), _sha(cam)
            if driver is not None:
                driver.after_op(i, op)
        net.flush()
        if driver is not None:
            driver.after_steps()
        sha["params"], sha["grads"] = _sha(net.get_params()), _sha(net.get_grads())
        if device_loss:
            sha["last_loss"] = _sha(np.float32(net.last_loss()))
        for lname, ent in zip(names, layout):
            try:
                sha["out:" + lname] = _sha(net.layer_output(lname, (last_B,) + tuple(ent["out"])))
            except (KeyError, RuntimeError) as e:
                sha["out:" + lname] = _rc(e)
        try:
            sha["input_delta"] = _sha(net.input_delta((last_B,) + in_shape))
        except KeyError as e:
            sha["input_delta"] = _rc(e)
        T.cuda.synchronize()
        log = {k: cnt for k, (cnt, _) in capi.kernel_timing_report().items()} if driver is None else {}
    finally:
        if driver is None:
            capi.kernel_timing(0)
        if option:
            capi.set_option(option[0], old_option)
        for fn in SWITCHES.values():
            getattr(lib, fn)(1)
        net.close()
    return {"log": log, "sha": sha}


def trace_record(T, repeats=1):
    """{case: {"log", "sha"}} over CASES with IGEMM_AUTOTUNE=0 held by the caller; repeats > 1 (the maker): every case runs that often on
    a fresh net -> (record, [cases whose record does not repeat])"""
    rec, unstable = {}, []
    for name in sorted(CASES):
        got = [run_case(T, name) for _ in range(repeats)]
        if any(g != got[0] for g in got):
            unstable.append(name)
        rec[name] = got[0]
    return rec, unstable
