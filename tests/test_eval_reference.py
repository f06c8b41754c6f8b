"""Device-side evaluation without a device: the NumPy restatement of cnn_eval_accumulate (tests/eval_ref.py) against CPU torch and on
hand-made cases, the exported / declared / bound names, every refusal of the new C ABI entries, the size of the state block."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.eval_ref import ref_accumulate, ref_batch, ref_loss_term, ref_predict, ref_rank
from tests.util import REL_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def seeded(B, classes, seed):
    """normal logits (scale 3) and labels in range; asserted tie-free and with a spread under 50, so that clamped_exp never clamps and
    torch's softmax is the same function"""
    rs = np.random.RandomState(seed)
    logits = (rs.standard_normal((B, classes)) * 3).astype(F)
    labels = rs.randint(0, classes, size=B).astype(np.int32)
    for row in logits:
        assert len(np.unique(row)) == classes, "tie"
    assert float((logits.max(axis=1) - logits.min(axis=1)).max()) < 50.0
    return logits, labels


@pytest.mark.parametrize("B,classes,k", [(257, 3, 2), (64, 10, 5), (33, 64, 1), (5, 1, 1), (17, 8, 8)])
def test_restatement_equals_cpu_torch(B, classes, k):
    import torch
    import torch.nn.functional as Fn

    logits, labels = seeded(B, classes, 100 + B + classes)
    got = ref_batch(logits, labels, k)
    z, y = torch.from_numpy(logits), torch.from_numpy(labels).long()
    pred = z.argmax(dim=1)
    assert np.array_equal(got["pred"], pred.numpy().astype(np.int32))
    in_topk = (torch.topk(z, k, dim=1).indices == y[:, None]).any(dim=1)
    assert got["samples"] == B and got["ignored"] == 0
    assert got["top1"] == int((pred == y).sum()) and got["topk"] == int(in_topk.sum())
    conf = torch.bincount(y * classes + pred, minlength=classes * classes).reshape(classes, classes).numpy()
    assert np.array_equal(got["confusion"], conf.astype(np.uint64))
    want = float(Fn.cross_entropy(z.double(), y, reduction="sum"))
    assert abs(float(got["loss_sum"]) - want) <= REL_TOL * abs(want), (float(got["loss_sum"]), want)


def test_tie_rule_lower_index_wins():
    z = np.array([1.0, 3.0, 3.0, 0.5, 3.0], F)
    assert ref_predict(z) == 1
    assert [ref_rank(z, y) for y in range(5)] == [3, 0, 1, 4, 2]
    labels = np.arange(5, dtype=np.int32)
    for k, topk in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 5)):
        got = ref_batch(np.tile(z, (5, 1)), labels, k)
        assert got["top1"] == 1 and got["topk"] == topk, (k, got)
    # all equal: the prediction is index 0, label j has rank j
    e = np.zeros(4, F)
    assert ref_predict(e) == 0 and [ref_rank(e, y) for y in range(4)] == [0, 1, 2, 3]


def test_k_equals_classes_counts_every_sample_and_one_class_is_always_right():
    logits, labels = seeded(19, 6, 7)
    got = ref_batch(logits, labels, 6)
    assert got["topk"] == got["samples"] == 19
    one = ref_batch(np.array([[2.5], [-7.0], [0.0]], F), np.zeros(3, np.int32), 1)
    assert one["top1"] == one["topk"] == one["samples"] == 3 and one["confusion"].tolist() == [[3]]
    assert float(one["loss_sum"]) == 0.0 and np.array_equal(one["pred"], [0, 0, 0])


def test_labels_out_of_range_are_ignored_only():
    logits, labels = seeded(6, 4, 3)
    padded = labels.copy()
    padded[[0, 3, 5]] = (-1, 4, -7)
    got = ref_batch(logits, padded, 2)
    kept = ref_batch(logits[[1, 2, 4]], labels[[1, 2, 4]], 2)
    assert got["ignored"] == 3 and got["samples"] == 3
    for key in ("top1", "topk"):
        assert got[key] == kept[key]
    assert np.array_equal(got["confusion"], kept["confusion"]) and got["loss_sum"].tobytes() == kept["loss_sum"].tobytes()
    assert np.array_equal(got["pred"], ref_batch(logits, labels, 2)["pred"])  # (predictions of ignored samples are still written)
    none = ref_batch(logits, np.full(6, -1, np.int32), 1)
    assert none["samples"] == 0 and none["ignored"] == 6 and int(none["confusion"].sum()) == 0 and float(none["loss_sum"]) == 0.0
    total = ref_accumulate([got, none, kept])
    assert (total["samples"], total["ignored"], total["top1"]) == (6, 9, 2 * kept["top1"])
    assert total["loss_sum"] == np.float64(got["loss_sum"]) + np.float64(kept["loss_sum"])


def test_nan_logits():
    nan = F("nan")
    first = np.array([nan, 1.0, 2.0], F)   # nothing is greater than a NaN maximum: the prediction stays 0
    later = np.array([1.0, nan, 0.5], F)   # a NaN elsewhere is never the prediction
    assert ref_predict(first) == 0 and ref_predict(later) == 0
    assert ref_rank(first, 2) == 0 and ref_rank(first, 1) == 1 and ref_rank(later, 2) == 1
    assert ref_rank(later, 1) == 0  # (a NaN label logit: no comparison holds; top-1 is still pred == label)
    got = ref_batch(np.stack([first, later, later]), np.array([0, 1, 0], np.int32), 1)
    assert np.array_equal(got["pred"], [0, 0, 0]) and got["top1"] == 2 and got["topk"] == 3
    # the row's maximum is the NaN: every exp is of a NaN, the sum is a NaN, p is NaN -> 0, the term log(0)
    assert ref_loss_term(first, 1) == -np.inf
    # a NaN elsewhere poisons the sum only: p is NaN -> 0 for every label
    assert ref_loss_term(later, 0) == -np.inf and ref_loss_term(later, 1) == -np.inf


NEW_ABI = ("cnn_eval_state_bytes", "cnn_eval_accumulate", "cnn_eval_read")
NEW_HOST = ("cnnh_net_eval_begin", "cnnh_net_eval_step_device", "cnnh_net_eval_result", "cnnh_net_get_predictions")


def test_new_names_are_exported_declared_and_bound():
    from cnn_amd import capi, hostapi

    lib, hlib = capi.load(), hostapi.load()
    hdr = open(os.path.join(ROOT, "include", "cnn_amd.h")).read()
    arch = open(os.path.join(ROOT, "cnn_amd", "host", "include", "architectures.h")).read()
    for name in NEW_ABI:
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    assert "typedef struct cnn_eval_result" in hdr and C.sizeof(capi.EvalResult) == 40
    for name in NEW_HOST:
        assert hasattr(hlib, name) and name in hostapi.SIGNATURES, name
    for member in ("void eval_begin(int top_k = 1)", "void eval_step(", "EvalResult eval_result(", "last_predictions_device() const", "struct EvalResult"):
        assert member in arch, member
    for name in ("eval_begin", "eval_step", "eval_result", "predictions", "evaluate"):
        assert callable(getattr(hostapi.HostNet, name)), name
    for name in ("eval_state_bytes", "eval_accumulate", "eval_read"):
        assert callable(getattr(capi, name)), name
    assert lib.cnn_amd_abi_version() == 2


def test_state_block_size():
    from cnn_amd import capi

    lib = capi.load()
    assert lib.cnn_eval_state_bytes(3) == 8 * (4 + 1 + 9) == capi.eval_state_bytes(3)
    assert lib.cnn_eval_state_bytes(1) == 48 and lib.cnn_eval_state_bytes(1000) == 8 * (5 + 1000 * 1000)
    for bad in (0, -1):
        assert lib.cnn_eval_state_bytes(bad) == 0 and b"classes" in lib.cnn_amd_last_error()
    with pytest.raises(capi.CnnAmdError):
        capi.eval_state_bytes(0)


def test_every_refusal_is_badarg_with_a_message():
    """nothing here reaches a launch or a copy: the pointers are small non-null integers that are never dereferenced"""
    from cnn_amd import capi

    lib = capi.load()
    p, q, r, s = (C.c_void_p(0x1000 * i) for i in (1, 2, 3, 4))

    def refused(rc, word):
        assert rc == 1, (rc, word)  # CNN_AMD_E_BADARG
        msg = lib.cnn_amd_last_error().decode()
        assert "cnn_eval_" in msg and word in msg, (word, msg)

    acc = lib.cnn_eval_accumulate
    refused(acc(None, q, r, s, 4, 3, 1, None), "null")
    refused(acc(p, None, r, s, 4, 3, 1, None), "null")
    refused(acc(p, q, r, None, 4, 3, 1, None), "null")
    refused(acc(p, q, None, None, 4, 3, 1, None), "null")  # (pred alone may be null; here the state is missing)
    for B in (0, -4):
        refused(acc(p, q, r, s, B, 3, 1, None), "B=")
    for classes in (0, -3):
        refused(acc(p, q, r, s, 4, classes, 1, None), "classes=")
    for k in (0, -1, 4):
        refused(acc(p, q, r, s, 4, 3, k, None), "k=")
    out = capi.EvalResult()
    read = lib.cnn_eval_read
    refused(read(None, 3, C.byref(out), None, None), "null")
    refused(read(p, 3, None, None, None), "null")
    for classes in (0, -1):
        refused(read(p, classes, C.byref(out), None, None), "classes=")
