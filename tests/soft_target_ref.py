"""NumPy restatements of the soft-target entries of include/cnn_amd.h: cnn_soft_targets and cnn_batch_mix in fp32 with the header's
operation order (every operation rounded on its own), the soft loss and its delta in float64.  tests/test_soft_targets_reference.py
holds them against CPU torch; the GPU tests hold the kernels against them bit for bit."""
import numpy as np

PAIR_NONE, PAIR_FLIP, PAIR_ROLL = 0, 1, 2
MIX_MIXUP, MIX_CUTMIX = 1, 2
F = np.float32


def ref_partner(B, rule, shift=0):
    """p(b) for every b; PAIR_NONE pairs every sample with itself"""
    b = np.arange(B)
    if rule == PAIR_FLIP:
        return B - 1 - b
    if rule == PAIR_ROLL:
        assert 1 <= shift < B
        return (b + shift) % B
    return b


def ref_base(labels, classes, smoothing):
    """base(l, j): one-hot rows at smoothing 0, (1 - s) + s / classes at the label and s / classes elsewhere otherwise; a label outside
    [0, classes) matches no column"""
    labels = np.asarray(labels, np.int64)
    hit = labels[:, None] == np.arange(classes)[None, :]
    if F(smoothing) == 0:
        return np.where(hit, F(1), F(0)).astype(F)
    u = F(smoothing) / F(classes)
    hot = (F(1) - F(smoothing)) + u
    return np.where(hit, hot, u).astype(F)


def ref_soft_targets(labels, classes, smoothing=0.0, lam=1.0, rule=PAIR_NONE, shift=0):
    base = ref_base(labels, classes, smoothing)
    if rule == PAIR_NONE or F(lam) == 1:
        return base
    oml = F(1) - F(lam)
    own = F(lam) * base
    other = oml * base[ref_partner(len(base), rule, shift)]
    return (own + other).astype(F)


def ref_cutmix_lambda(H, W, y0, y1, x0, x1):
    return F(1.0 - float((y1 - y0) * (x1 - x0)) / (float(H) * W))


def ref_batch_mix(x, mode, lam=1.0, rule=PAIR_NONE, shift=0, box=(0, 0, 0, 0)):
    """x float32 [B][C][H][W]; box = (y0, y1, x0, x1).  The copies keep every bit (the array is moved as uint32 there)."""
    x = np.ascontiguousarray(x, F)
    y0, y1, x0, x1 = box
    if rule == PAIR_NONE or (mode == MIX_MIXUP and F(lam) == 1) or (mode == MIX_CUTMIX and (y0 == y1 or x0 == x1)):
        return x.copy()
    partner = x[ref_partner(x.shape[0], rule, shift)]
    if mode == MIX_MIXUP:
        oml = F(1) - F(lam)
        with np.errstate(invalid="ignore", over="ignore"):
            return ((F(lam) * x) + (oml * partner)).astype(F)
    out = x.view(np.uint32).copy()
    out[:, :, y0:y1, x0:x1] = partner.view(np.uint32)[:, :, y0:y1, x0:x1]
    return out.view(F)


def ref_soft_loss(logits, targets):
    """float64: (mean_b(-sum_j t_j log_softmax_j), softmax - t, sum_b sum_j |t_j log_softmax_j|)"""
    z = np.asarray(logits, np.float64)
    t = np.asarray(targets, np.float64)
    z = z - z.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    terms = t * logp
    return float(-terms.sum() / z.shape[0]), np.exp(logp) - t, float(np.abs(terms).sum())
