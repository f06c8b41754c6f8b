"""cnn_eval_accumulate / cnn_eval_read (include/cnn_amd.h) on the device, through cnn_amd.capi.  The integers and the predictions are
held exactly to the NumPy restatement (tests/eval_ref.py); the batch loss sum is held bit for bit to cnn_softmax_xent(probs = NULL)
on the same logits -- with ignored labels, on the batch without those samples -- and, as a sanity bound, to the restatement at
REL_TOL.  Operands and outputs live between poisoned guard zones (tests/guarded.py); the logits of every second label pattern start
4 bytes past a 16-byte boundary.  The references come from the host once per shape."""
import functools

import numpy as np
import pytest

from tests import guarded
from tests.conv_route_cases import _logged
from tests.eval_ref import ref_accumulate, ref_batch, ref_samples
from tests.util import REL_TOL

pytestmark = pytest.mark.gpu

# B: a partial workgroup (1, 2, 255), exactly one full trip (256), a second trip (257, 600); classes: 1, 2, odd, 8 / 9 around the fused
# head's limit, 64; and 1000 classes once
SHAPES = [(B, c) for B in (1, 2, 255, 256, 257, 600) for c in (1, 2, 3, 8, 9, 64)] + [(33, 1000)]


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def make_logits(B, classes, seed):
    """normal logits (scale 3, spread far under 50: clamped_exp never clamps, no probability underflows); in every fourth row one
    class's logit is copied to another (an exact tie), in every eighth of them it is the row's maximum that is copied"""
    rs = np.random.RandomState(seed)
    z = (rs.standard_normal((B, classes)) * 3).astype(np.float32)
    if classes >= 2:
        for b in range(0, B, 4):
            src = int(np.argmax(z[b])) if b % 8 == 0 else int(rs.randint(classes))
            dst = (src + 1 + int(rs.randint(classes - 1))) % classes
            z[b, dst] = z[b, src]
    assert float((z.max(axis=1) - z.min(axis=1)).max()) < 50.0
    return z


def make_labels(B, classes, seed, pattern):
    rs = np.random.RandomState(seed + 1)
    y = rs.randint(0, classes, size=B).astype(np.int32)
    if pattern == "ignored":  # the first, a middle and the last sample: below, above, below the range
        y[0], y[B // 2], y[B - 1] = -1, classes, -5
    elif pattern == "all_ignored":
        y[:] = np.where(np.arange(B) % 2 == 0, -1, classes)
    return y


@functools.lru_cache(maxsize=None)
def reference(B, classes, pattern):
    """-> (logits, labels, ref_samples of them); computed once per shape and label pattern, never written"""
    z = make_logits(B, classes, 4000 + 7 * B + classes)
    y = make_labels(B, classes, 4000 + 7 * B + classes, pattern)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y, ref_samples(z, y)


def ks_of(classes):
    return sorted({1, min(2, classes), classes})


def fresh_state(T, classes, keep):
    """a state block between guards, cleared by cnn_memset_zero (the poison would be a state with 6e18 samples)"""
    from cnn_amd import capi

    st = guarded.output((capi.eval_state_bytes(classes),), guarded.BYTES, keep, "state", T.uint8)
    capi.check(capi.load().cnn_memset_zero(capi._ptr(st), st.numel(), capi._stream()), "cnn_memset_zero")
    return st


def run_once(T, logits_dev, labels_dev, classes, k, keep):
    """one cnn_eval_accumulate into a fresh state under the launch log -> (state tensor, pred tensor, log)"""
    from cnn_amd import capi

    st = fresh_state(T, classes, keep)
    pred = guarded.output((logits_dev.shape[0],), guarded.BYTES, keep, "pred", T.int32)
    def call():
        capi.eval_accumulate(logits_dev, labels_dev, st, k, pred)
        return {}

    return st, pred, _logged(T, call)["log"]


def xent_loss(T, logits, labels):
    """cnn_softmax_xent(probs = NULL)'s fp32 loss_sum on the samples whose label is in range; None when there is none"""
    from cnn_amd import capi

    classes = logits.shape[1]
    keep = (labels >= 0) & (labels < classes)
    if not keep.any():
        return None
    zd = T.from_numpy(np.ascontiguousarray(logits[keep])).cuda()
    yd = T.from_numpy(np.ascontiguousarray(labels[keep])).cuda()
    _, _, loss = capi.softmax_xent(zd, yd, want_probs=False)
    return loss.cpu().numpy()[0]


@pytest.mark.parametrize("B,classes", SHAPES)
def test_eval_kernel_equals_the_restatement_and_the_loss_kernel(T, B, classes):
    from cnn_amd import capi

    for i, pattern in enumerate(("clean", "ignored", "all_ignored")):
        z, y, samples = reference(B, classes, pattern)
        keep = []
        zd = guarded.operand(z, guarded.POISONS[i % 2], keep, "logits", shift_bytes=4 * (i % 2))
        yd = guarded.operand(y, guarded.BYTES, keep, "labels")
        assert zd.data_ptr() % 16 == 4 * (i % 2)
        want_loss = xent_loss(T, z, y)
        for k in ks_of(classes) if pattern != "all_ignored" else [1]:
            ref = ref_batch(z, y, k, samples)
            st, pred, log = run_once(T, zd, yd, classes, k, keep)
            assert len(log) == 1 and all(name.startswith("eval_") and cnt == 1 for name, cnt in log.items()), log
            got = capi.eval_read(st, classes)
            what = (B, classes, pattern, k)
            assert np.array_equal(pred.cpu().numpy(), ref["pred"]), what
            for key in ("samples", "top1", "topk", "ignored"):
                assert got[key] == ref[key], (what, key, got[key], ref[key])
            assert np.array_equal(got["confusion"], ref["confusion"]), what
            # one call into an empty state: loss_sum = 0.0 + (double)batch_sum, which keeps every bit of a batch sum but the sign of a zero
            # (one class: every term is log(1)); the loss kernel's fp32 value goes through the same sum
            batch = np.float32(got["loss_sum"])
            print(f"B {B} classes {classes} {pattern} k {k}: loss sum {batch!r}, loss kernel {want_loss!r}, restatement {ref['loss_sum']!r}")
            assert np.float64(batch) == got["loss_sum"], what
            if want_loss is None:
                assert got["loss_sum"] == 0.0 and got["samples"] == 0, what
            else:
                assert np.float64(got["loss_sum"]).tobytes() == (np.float64(0) + np.float64(want_loss)).tobytes(), (what, batch, want_loss)
                assert abs(float(batch) - float(ref["loss_sum"])) <= REL_TOL * abs(float(ref["loss_sum"])), (what, batch, ref["loss_sum"])
            # the same call again: the same bytes
            st2, pred2, _ = run_once(T, zd, yd, classes, k, keep)
            assert T.equal(st, st2) and T.equal(pred, pred2), what
        assert guarded.check(keep) == [], (B, classes, pattern)


def test_cleared_state_reads_as_zeros(T):
    from cnn_amd import capi

    keep = []
    got = capi.eval_read(fresh_state(T, 9, keep), 9)
    assert [got[key] for key in ("samples", "top1", "topk", "ignored")] == [0, 0, 0, 0] and got["loss_sum"] == 0.0
    assert not got["confusion"].any() and guarded.check(keep) == []
    assert capi.eval_read(fresh_state(T, 9, keep), 9, want_confusion=False).keys() == {"samples", "top1", "topk", "ignored", "loss_sum"}


@pytest.mark.parametrize("classes,k", [(3, 1), (9, 2), (64, 64)])
def test_four_calls_into_one_state(T, classes, k):
    """batches of 257, 2, 600 and 255 samples -- clean, with ignored samples, all ignored, clean -- into ONE state: the integers are the
    sums, loss_sum is the fp64 sum of the four fp32 batch sums (each read from a call of its own) in call order, bit for bit"""
    from cnn_amd import capi

    plan = [(257, "clean"), (2, "ignored"), (600, "all_ignored"), (255, "clean")]
    keep, singles, refs = [], [], []
    st = fresh_state(T, classes, keep)
    for B, pattern in plan:
        z, y, samples = reference(B, classes, pattern)
        zd, yd = guarded.operand(z, guarded.NAN, keep, "logits"), guarded.operand(y, guarded.BYTES, keep, "labels")
        own, _, _ = run_once(T, zd, yd, classes, k, keep)
        singles.append(np.float32(capi.eval_read(own, classes, want_confusion=False)["loss_sum"]))
        capi.eval_accumulate(zd, yd, st, k)  # (pred is optional)
        refs.append(ref_batch(z, y, k, samples))
    got = capi.eval_read(st, classes)
    want = ref_accumulate(refs)
    for key in ("samples", "top1", "topk", "ignored"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert np.array_equal(got["confusion"], want["confusion"])
    total = np.float64(0)
    for s in singles:
        total = np.float64(total + np.float64(s))
    assert np.float64(got["loss_sum"]).tobytes() == total.tobytes(), (got["loss_sum"], total)
    assert guarded.check(keep) == []
