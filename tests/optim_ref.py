"""Host reference of the optimizer step (cnn_sgd_momentum_update, include/cnn_amd.h) and of the container's decay policy
(Sequential::set_optimizer).  NumPy only; every intermediate is an np.float32 array, so every product and sum is rounded separately
-- the arithmetic the kernel is held to bit for bit."""
import numpy as np


def ref_sgd_step(p, g, v, lr, momentum=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0, decay_ranges=()):
    """one step over flat fp32 arrays -> (p', v').  decay_ranges: [(begin, end)] half-open index ranges weight decay applies to.
        gs = g * grad_scale            (only when grad_scale != 1)
        d  = gs + weight_decay * p     (inside the ranges, only when weight_decay != 0; gs elsewhere)
        momentum == 0:  u = d          (v comes back untouched)
        otherwise:      v' = momentum * v + d;  u = d + momentum * v' (nesterov) or v'
        p' = p - lr * u"""
    f = np.float32
    p = np.asarray(p, f)
    g = np.asarray(g, f)
    assert p.ndim == 1 and p.shape == g.shape
    lr, momentum, weight_decay, grad_scale = f(lr), f(momentum), f(weight_decay), f(grad_scale)
    gs = g * grad_scale if grad_scale != f(1) else g
    assert gs.dtype == f
    d = gs.copy()
    if weight_decay != f(0):
        mask = np.zeros(p.size, bool)
        for b, e in decay_ranges:
            mask[int(b):int(e)] = True
        wp = weight_decay * p
        d[mask] = (gs + wp)[mask]
    if momentum == f(0):
        u, v_new = d, v
    else:
        v = np.asarray(v, f)
        assert v.shape == p.shape
        mv = momentum * v
        v_new = mv + d
        if nesterov:
            mvn = momentum * v_new
            u = d + mvn
        else:
            u = v_new
    step = lr * u
    p_new = p - step
    assert p_new.dtype == f and d.dtype == f and step.dtype == f
    return p_new, v_new


def decay_ranges_of(layout, bias_and_norm=False):
    """the decayed index ranges of a cnn_amd.stacks.walk() layout in arena (= checkpoint) order, neighbours merged: Conv2D and
    LinearLayer weights; with bias_and_norm also their biases and BatchNorm2D's gamma / beta; never moving_mean / moving_var"""
    out, off = [], 0
    for e in layout:
        n = e["params"]
        r = None
        if e["kind"] == "conv":
            r = (off, off + (n if bias_and_norm else n - e["Co"]))
        elif e["kind"] == "linear":
            r = (off, off + (n if bias_and_norm else n - e["n_out"]))
        elif e["kind"] == "bn" and bias_and_norm:
            r = (off, off + n // 2)
        if r is not None:
            if out and out[-1][1] == r[0]:
                out[-1] = (out[-1][0], r[1])
            else:
                out.append(r)
        off += n
    return out


def moving_stat_mask(layout):
    """True at the arena positions of BatchNorm2D's moving_mean / moving_var"""
    mask, off = [], 0
    for e in layout:
        n = e["params"]
        m = np.zeros(n, bool)
        if e["kind"] == "bn":
            m[n // 2:] = True
        mask.append(m)
        off += n
    return np.concatenate(mask) if mask else np.zeros(0, bool)
