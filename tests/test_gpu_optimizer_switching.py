"""Every switch between the container's five optimizer kinds -- the plain step (set_optimizer(0, 0)), momentum SGD, Adam, LAMB, LARS --
as an ordered pair (A, B): one train_step under A, one under B, then save_optimizer_state.  What the state file, the launch log, the
state arenas and the step counter show must be B's and only B's, and A's state must have survived.  Nothing here depends on how the
container stores "which optimizer is active"; the C boundary exposes layerwise_active() alone of the *_active() accessors, so the
kind is read from the three places a caller can see it: layerwise_active(), the kernels of the step and the magic of the state file."""
import struct

import numpy as np
import pytest

from tests.test_gpu_optimizer import LR, make_net, net_inputs, same, step_kernels

pytestmark = pytest.mark.gpu

STEP_FAMILIES = ("sgd_", "sgdm_", "adam_", "lamb_", "lars_", "seg_", "clip_")  # every kernel an arena step can launch


def _arm_plain(net):
    net.set_optimizer(0, 0)


# arm: non-default options; header: struct format behind magic + n_params and the values it must unpack to; families: the step's kernels;
# arenas: the state the kind's file carries (and its step writes); counts: the step counter advances under it
KINDS = {
    "plain": dict(arm=_arm_plain, magic=b"CNNAOPT1", fmt="<ffII", header=(0.0, 0.0, 0, 0), families={"sgd_"}, arenas=("velocity",), uses=(),
                  counts=False),
    "sgdm": dict(arm=lambda net: net.set_optimizer(0.8, 2e-3, nesterov=True, decay_bias_and_norm=True), magic=b"CNNAOPT1", fmt="<ffII",
                 header=(0.8, 2e-3, 1, 1), families={"sgdm_"}, arenas=("velocity",), uses=("velocity",), counts=False),
    "adam": dict(arm=lambda net: net.set_adam(0.8, 0.99, 1e-6, 3e-3, decoupled=True, decay_bias_and_norm=True), magic=b"CNNAADM1", fmt="<QffffII",
                 header=(None, 0.8, 0.99, 1e-6, 3e-3, 1, 1), families={"adam_"}, arenas=("m", "v"), uses=("m", "v"), counts=True),
    "lamb": dict(arm=lambda net: net.set_lamb(0.85, 0.98, 1e-5, 2e-2, decay_bias_and_norm=True, adapt_bias_and_norm=True), magic=b"CNNALMB1",
                 fmt="<QffffII", header=(None, 0.85, 0.98, 1e-5, 2e-2, 1, 1), families={"lamb_", "seg_"}, arenas=("m", "v"), uses=("m", "v"),
                 counts=True),
    "lars": dict(arm=lambda net: net.set_lars(0.7, 1e-3, trust_coefficient=2e-3, eps=1e-7, nesterov=True, decay_bias_and_norm=True,
                                              adapt_bias_and_norm=False), magic=b"CNNALRS1", fmt="<ffffIIII",
                 header=(0.7, 1e-3, 2e-3, 1e-7, 1, 1, 0, 0), families={"lars_", "seg_"}, arenas=("velocity",), uses=("velocity",), counts=False),
}


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture(scope="module")
def inputs(T):
    return net_inputs(T, "small_bn", 610)


def pointers(net):
    m, v = net.adam_ptrs()
    return {"velocity": net.velocity_ptr(), "m": m, "v": v}


def arenas_of(net, names):
    out = {}
    if "velocity" in names:
        out["velocity"] = net.get_velocity()
    if "m" in names:
        out["m"], out["v"], _ = net.get_adam_state()
    return out


def step_counter(net):
    return net.get_adam_state()[2] if net.adam_ptrs()[0] else 0


def families_in(log):
    return {f for f in STEP_FAMILIES for k in log if k.startswith(f)}


def f32(x):
    return float(np.float32(x))


@pytest.mark.parametrize("kind_b", list(KINDS))
@pytest.mark.parametrize("kind_a", list(KINDS))
def test_switch(T, inputs, tmp_path, kind_a, kind_b):
    layout, p0, x, labels = inputs
    A, B = KINDS[kind_a], KINDS[kind_b]
    net = make_net("small_bn")
    net.set_params(p0)
    A["arm"](net)
    ptrs_a = pointers(net)
    assert all(ptrs_a[name] for name in A["arenas"])
    net.train_step(x, labels, LR)
    assert step_counter(net) == int(A["counts"])
    state_a = arenas_of(net, A["arenas"])
    assert all(np.any(state_a[name]) for name in A["uses"]) and not any(np.any(state_a[name]) for name in set(A["arenas"]) - set(A["uses"]))
    B["arm"](net)
    # the switch itself frees, moves and zeroes nothing
    ptrs_b = pointers(net)
    assert all(ptrs_b[name] == ptrs_a[name] for name in A["arenas"]) and all(ptrs_b[name] for name in B["arenas"])
    assert all(same(arr, state_a[name]) for name, arr in arenas_of(net, A["arenas"]).items())
    assert step_counter(net) == int(A["counts"])
    log = step_kernels(T, net, x, labels, steps=1)
    assert families_in(log) == B["families"], (kind_a, kind_b, sorted(k for k in log if k.startswith(STEP_FAMILIES)))
    assert net.layerwise_active() == (kind_b in ("lamb", "lars"))
    assert step_counter(net) == int(A["counts"]) + int(B["counts"])
    assert pointers(net) == ptrs_b
    for name, arr in arenas_of(net, A["arenas"]).items():
        if name in B["uses"]:  # (Adam <-> LAMB share the moments, momentum SGD <-> LARS the velocity: B's step moved it on)
            assert not same(arr, state_a[name]), name
        else:
            assert same(arr, state_a[name]), name
    path = str(tmp_path / "b.state")
    assert net.lib.cnnh_net_save_optimizer_state(net.h, path.encode()) == 0
    blob = open(path, "rb").read()
    n = net.n_params
    head = 16 + struct.calcsize(B["fmt"])
    assert blob[:8] == B["magic"] and struct.unpack("<Q", blob[8:16])[0] == n
    assert head == (32 if B["magic"] == b"CNNAOPT1" else 48) and len(blob) == head + len(B["arenas"]) * 4 * n
    fields = struct.unpack(B["fmt"], blob[16:head])
    want = tuple(step_counter(net) if w is None else (f32(w) if isinstance(w, float) else w) for w in B["header"])
    assert fields == want, (fields, want)
    payload = np.frombuffer(blob[head:], np.float32)
    now = arenas_of(net, B["arenas"])
    assert same(payload, np.concatenate([now[name] for name in B["arenas"]]))
    net.close()


def test_a_net_that_never_had_an_optimizer_has_no_state_to_save(T, inputs, tmp_path):
    layout, p0, x, labels = inputs
    net = make_net("small_bn")
    net.set_params(p0)
    log = step_kernels(T, net, x, labels, steps=1)
    assert families_in(log) == {"sgd_"}
    path = tmp_path / "none.state"
    assert net.lib.cnnh_net_save_optimizer_state(net.h, str(path).encode()) == 4 and not path.exists()
    assert pointers(net) == {"velocity": None, "m": None, "v": None} and not net.layerwise_active() and net.segment_count() == 0
    net.close()


def test_adam_lars_adam_on_the_fused_tail(T):
    """the reference net at B = 16 (pool-fused front block, fused step tail): Adam -> LARS -> Adam with one step after each.  The
    layer-wise step in the middle takes the plain sequence; the third step is back on the fused tail -- two adam launches, one per
    range, carrying ONE step number -- and no layer-wise kernel is left in it."""
    layout, p0, x, labels = net_inputs(T, "alexnet", 620)
    net = make_net("alexnet")
    net.set_params(p0)
    net.set_adam(weight_decay=1e-2)
    net.train_step(x, labels, LR)
    assert step_counter(net) == 1
    net.set_lars(0.9, 5e-4)
    log = step_kernels(T, net, x, labels, steps=1)
    assert families_in(log) == {"lars_", "seg_"} and step_counter(net) == 1
    net.set_adam(weight_decay=1e-2)
    log = step_kernels(T, net, x, labels, steps=1)
    assert sum(cnt for k, cnt in log.items() if k.startswith("adam_")) == 2, log
    assert families_in(log) == {"adam_"}, log
    assert step_counter(net) == 2 and not net.layerwise_active()
    net.close()
