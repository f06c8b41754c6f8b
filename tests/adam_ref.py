"""Host reference of the Adam / AdamW step (cnn_adam_update, include/cnn_amd.h) and of the clip by the global gradient norm
(cnn_clip_grad_norm).  NumPy only; every intermediate is an np.float32 array, so every product, sum, quotient and root is rounded
separately (NumPy's fp32 division and square root are the correctly rounded IEEE operations) -- the arithmetic the kernels are held to
bit for bit."""
import math

import numpy as np


def adam_host_scalars(step, lr, beta1, beta2, weight_decay):
    """(om, omb1, omb2, bc2s, ss) as the entry point computes them: the options are fp32 values, the bias corrections go through
    double-precision pow / sqrt and are narrowed once"""
    f = np.float32
    lr, beta1, beta2, weight_decay = f(lr), f(beta1), f(beta2), f(weight_decay)
    lw = f(lr * weight_decay)
    om = f(f(1) - lw)
    omb1 = f(f(1) - beta1)
    omb2 = f(f(1) - beta2)
    bc2s = f(math.sqrt(1.0 - math.pow(float(beta2), float(int(step)))))
    ss = f(float(lr) / (1.0 - math.pow(float(beta1), float(int(step)))))
    return om, omb1, omb2, bc2s, ss


def ref_adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, grad_scale=1.0,
                  decay_ranges=()):
    """one step over flat fp32 arrays -> (p', m', v').  step: the 1-based number of this step.  decay_ranges: [(begin, end)] half-open
    index ranges weight decay applies to.
        gs  = g * grad_scale                      (only when grad_scale != 1)
        d   = gs + weight_decay * p               (inside the ranges, weight_decay != 0, not decoupled; gs elsewhere)
        p0  = p * om                              (inside the ranges, weight_decay != 0, decoupled; p elsewhere)
        m'  = beta1 * m + omb1 * d
        v'  = beta2 * v + omb2 * (d * d)
        den = sqrt(v') / bc2s + eps
        p'  = p0 - ss * (m' / den)"""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    assert p.ndim == 1 and p.shape == g.shape == m.shape == v.shape and int(step) >= 1
    om, omb1, omb2, bc2s, ss = adam_host_scalars(step, lr, beta1, beta2, weight_decay)
    beta1, beta2, eps, weight_decay, grad_scale = f(beta1), f(beta2), f(eps), f(weight_decay), f(grad_scale)
    gs = g * grad_scale if grad_scale != f(1) else g
    d = gs.copy()
    p0 = p.copy()
    if weight_decay != f(0):
        mask = np.zeros(p.size, bool)
        for b, e in decay_ranges:
            mask[int(b):int(e)] = True
        if decoupled:
            p0[mask] = (p * om)[mask]
        else:
            wp = weight_decay * p
            d[mask] = (gs + wp)[mask]
    with np.errstate(all="ignore"):
        b1m = beta1 * m
        o1d = omb1 * d
        m_new = b1m + o1d
        b2v = beta2 * v
        dd = d * d
        o2d = omb2 * dd
        v_new = b2v + o2d
        root = np.sqrt(v_new)
        rb = root / bc2s
        den = rb + eps
        q = m_new / den
        stp = ss * q
        p_new = p0 - stp
    for a in (gs, d, p0, b1m, o1d, m_new, b2v, dd, o2d, v_new, root, rb, den, q, stp, p_new):
        assert a.dtype == f
    return p_new, m_new, v_new


def ref_clip(g, norm_f32, max_norm, grad_scale=1.0):
    """cnn_clip_grad_norm from a given fp32 norm -> (g', coef):
        total = norm * grad_scale (only when grad_scale != 1);  c = max_norm / (total + 1e-6);  coef = c < 1 ? c : 1 (a NaN total: 1);
        g' = g * coef only when coef < 1
    Starting from the device's own stats[0] -- which has grad_scale folded in already -- pass grad_scale = 1."""
    f = np.float32
    g = np.asarray(g, f)
    with np.errstate(all="ignore"):
        total = f(f(norm_f32) * f(grad_scale)) if f(grad_scale) != f(1) else f(norm_f32)
        s = f(total + f(1e-6))
        c = f(f(max_norm) / s)
    coef = c if c < f(1) else f(1)
    if coef < f(1):
        out = g * coef
        assert out.dtype == f
        return out, coef
    return g.copy(), coef


def ref_total_norm(g, grad_scale=1.0):
    """the fp64 value the device's stats[0] is held to: (float)sqrt(sum of squares in double), times grad_scale in fp32"""
    f = np.float32
    norm = f(np.sqrt(np.sum(np.asarray(g, f).astype(np.float64) ** 2)))
    return f(norm * f(grad_scale)) if f(grad_scale) != f(1) else norm
