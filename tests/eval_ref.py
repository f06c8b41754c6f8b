"""NumPy restatement of cnn_eval_accumulate (include/cnn_amd.h): prediction, rank, ignored labels and confusion as plain loops and
comparisons, the loss term in the kernel's fp32 expressions and order, the bookkeeping over several calls in fp64.  The integers are
exact; the loss term goes through NumPy's fp32 exp and log, which may differ from the device's by an ulp, so tests compare the loss at
tests.util.REL_TOL and take bit-exactness from cnn_softmax_xent on the device instead.
A plain module: tests import it (`from tests.eval_ref import ...`)."""
import numpy as np

F = np.float32


def clamped_exp(v):
    """func.cpp:6-12 in fp32"""
    if v >= F(88):
        return np.finfo(F).max
    if v <= F(-50):
        return F(0)
    return np.exp(F(v))


def ref_predict(z):
    """the first maximum, strict '>' from index 0 (a NaN is never greater)"""
    best, mx = 0, z[0]
    for i in range(1, len(z)):
        if z[i] > mx:
            best, mx = i, z[i]
    return best


def ref_rank(z, y):
    """#{j : z[j] > z[y]} + #{j < y : z[j] == z[y]}"""
    return sum(1 for j in range(len(z)) if z[j] > z[y]) + sum(1 for j in range(y) if z[j] == z[y])


def ref_loss_term(z, y):
    """logf(p[y]): sequential max, sequential sum of the clamped exp, one quotient, NaN -> 0 -- every operation rounded to fp32"""
    with np.errstate(all="ignore"):
        mx = z[0]
        for i in range(1, len(z)):
            if z[i] > mx:
                mx = z[i]
        s = F(0)
        for i in range(len(z)):
            s = F(s + clamped_exp(F(z[i] - mx)))
        p = F(clamped_exp(F(z[y] - mx)) / s)
        if np.isnan(p):
            p = F(0)
        return F(np.log(p))


def ref_samples(logits, labels):
    """what does not depend on k, per sample: (pred int32 [B], rank int [B] with -1 for an ignored sample, term fp32 [B])"""
    logits = np.asarray(logits, F)
    B, classes = logits.shape
    pred, rank, term = np.zeros(B, np.int32), np.full(B, -1, np.int64), np.zeros(B, F)
    for b in range(B):
        z, y = logits[b], int(labels[b])
        pred[b] = ref_predict(z)
        if 0 <= y < classes:
            rank[b] = ref_rank(z, y)
            term[b] = ref_loss_term(z, y)
    return pred, rank, term


def ref_batch(logits, labels, k, samples=None):
    """one call: {"pred" int32 [B], "samples", "top1", "topk", "ignored", "confusion" uint64 [classes][classes], "loss_sum" fp32 (the
    terms of the non-ignored samples added in ascending sample order in fp32, negated)}; samples: ref_samples of the same batch, where
    a test asks for several k"""
    logits = np.asarray(logits, F)
    B, classes = logits.shape
    assert 1 <= k <= classes
    pred, rank, term = ref_samples(logits, labels) if samples is None else samples
    out = {"pred": pred, "samples": 0, "top1": 0, "topk": 0, "ignored": 0, "confusion": np.zeros((classes, classes), np.uint64)}
    running = F(0)
    with np.errstate(all="ignore"):
        for b in range(B):
            y = int(labels[b])
            if y < 0 or y >= classes:
                out["ignored"] += 1
                continue
            out["samples"] += 1
            out["top1"] += int(pred[b] == y)
            out["topk"] += int(rank[b] < k)
            out["confusion"][y, pred[b]] += np.uint64(1)
            running = F(running + term[b])
        out["loss_sum"] = F(-running)
    return out


def ref_accumulate(calls):
    """the state after a sequence of calls [(result of ref_batch, or any dict with its keys), ...]: the integers added, loss_sum the fp64
    sum of the fp32 batch sums in call order"""
    first = calls[0]
    total = {"samples": 0, "top1": 0, "topk": 0, "ignored": 0, "loss_sum": np.float64(0), "confusion": np.zeros_like(first["confusion"])}
    with np.errstate(all="ignore"):
        for c in calls:
            for key in ("samples", "top1", "topk", "ignored"):
                total[key] += int(c[key])
            total["confusion"] += c["confusion"]
            total["loss_sum"] = np.float64(total["loss_sum"] + np.float64(F(c["loss_sum"])))
    return total
