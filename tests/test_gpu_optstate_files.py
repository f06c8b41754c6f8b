"""The four optimizer state formats (CNNAOPT1, CNNAADM1, CNNALMB1, CNNALRS1) against files written by the code that shipped them:
tests/golden/optstate_{sgd,adam,lamb,lars}.state, recorded once by tests/golden/make_optstate_kat.py at the commit named in
optstate_kat.json.  Loading a file activates its optimizer, options, step counter and arenas; saving again reproduces it byte for
byte; a damaged copy is refused with the documented status and changes nothing -- neither in a net that never had an optimizer nor
in one that runs another optimizer."""
import json
import os
import struct

import numpy as np
import pytest

from tests.lamb_ref import segment_table_of
from tests.test_gpu_optimizer import LR, make_net, net_inputs, same

pytestmark = pytest.mark.gpu

OTHER = {"sgd": "adam", "adam": "lars", "lamb": "sgd", "lars": "lamb"}  # the optimizer the refusing net runs


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture(scope="module")
def kat(golden_dir):
    return json.load(open(os.path.join(golden_dir, "optstate_kat.json")))


@pytest.fixture(scope="module")
def inputs(T, kat):
    return net_inputs(T, "small_bn", kat["seed"])


def pointers(net):
    return (net.velocity_ptr(),) + tuple(net.adam_ptrs())


def step_counter(net):
    return net.get_adam_state()[2] if net.adam_ptrs()[0] else 0


def load(net, path):
    return net.lib.cnnh_net_load_optimizer_state(net.h, str(path).encode())


def save(net, path):
    return net.lib.cnnh_net_save_optimizer_state(net.h, str(path).encode())


def damaged_copies(entry, blob, tmp_path):
    """(file, status load_optimizer_state must return)"""
    nan = struct.pack("<f", float("nan"))
    at = entry["first_option_at"]
    n_params = struct.unpack("<Q", blob[8:16])[0]
    cases = {"short": (blob[:-8], 2), "header_only": (blob[:entry["header_bytes"]], 2),
             "other_n_params": (blob[:8] + struct.pack("<Q", n_params + 1) + blob[16:], 3), "nan_option": (blob[:at] + nan + blob[at + 4:], 2)}
    out = []
    for name, (data, status) in cases.items():
        path = tmp_path / f"{name}.state"
        path.write_bytes(data)
        out.append((path, status))
    return out


@pytest.mark.parametrize("name", ["sgd", "adam", "lamb", "lars"])
def test_golden_state_file(T, kat, inputs, golden_dir, tmp_path, name):
    layout, p0, x, labels = inputs
    entry = kat["files"][name]
    golden = os.path.join(golden_dir, entry["file"])
    blob = open(golden, "rb").read()
    n, head = kat["n_params"], entry["header_bytes"]
    assert blob[:8] == entry["magic"].encode() and struct.unpack("<Q", blob[8:16])[0] == n and len(blob) == head + entry["arenas"] * 4 * n
    payload = np.frombuffer(blob[head:], np.float32)

    # ---- a fresh net takes over the file's optimizer, options, step counter and arenas, and writes the same file again
    net = make_net("small_bn")
    assert net.n_params == n
    net.set_params(p0)
    assert pointers(net) == (None, None, None)
    assert load(net, golden) == 0
    opts = entry["options"]
    assert net.layerwise_active() == (name in ("lamb", "lars"))
    if name in ("sgd", "lars"):
        assert net.velocity_ptr() and net.adam_ptrs() == (None, None) and same(net.get_velocity(), payload)
    else:
        m, v, step = net.get_adam_state()
        assert not net.velocity_ptr() and step == entry["step"] == kat["steps"] and same(np.concatenate([m, v]), payload)
    if name in ("lamb", "lars"):
        bounds, flags = segment_table_of(layout, opts["decay_bias_and_norm"], opts["adapt_bias_and_norm"])
        got = net.segment_table()
        assert np.array_equal(got[0], bounds) and np.array_equal(got[1], flags)
    else:
        assert net.segment_count() == 0
    again = tmp_path / "again.state"
    assert save(net, again) == 0 and again.read_bytes() == blob
    net.close()

    # ---- a damaged copy is refused; a net that never had an optimizer still has none
    bad = damaged_copies(entry, blob, tmp_path)
    fresh = make_net("small_bn")
    fresh.set_params(p0)
    for path, status in bad:
        assert load(fresh, path) == status, path.name
        assert pointers(fresh) == (None, None, None) and not fresh.layerwise_active() and fresh.segment_count() == 0, path.name
        assert save(fresh, tmp_path / "none.state") == 4, path.name
    fresh.close()

    # ---- ... and a net that runs another optimizer keeps it: kind, options, step counter and arenas (its own state file is unchanged)
    other = kat["files"][OTHER[name]]
    net = make_net("small_bn")
    net.set_params(p0)
    getattr(net, other["setter"])(**other["options"])
    net.train_step(x, labels, LR)
    before, ptrs, count, segs = tmp_path / "before.state", pointers(net), step_counter(net), net.segment_table()
    assert save(net, before) == 0 and before.read_bytes()[:8] == other["magic"].encode()
    for path, status in bad:
        assert load(net, path) == status, path.name
        after = tmp_path / "after.state"
        assert save(net, after) == 0 and after.read_bytes() == before.read_bytes(), path.name
        assert pointers(net) == ptrs and step_counter(net) == count, path.name
        assert net.layerwise_active() == (OTHER[name] in ("lamb", "lars")), path.name
        assert all(np.array_equal(a, b) for a, b in zip(net.segment_table(), segs)), path.name
    net.close()
