"""Host reference of the layer-wise optimizers (cnn_lamb_update, cnn_lars_update, cnn_segment_norms; include/cnn_amd.h) and of the
container's segment table (Sequential::set_lamb / set_lars).  NumPy only; every intermediate is an np.float32 array, so every product,
sum, quotient and root is rounded separately (NumPy's fp32 division and square root are the correctly rounded IEEE operations) -- the
arithmetic the kernels are held to bit for bit.  The updates TAKE the segment norms as an argument: the device's fp64 sums differ
from NumPy's only in their order, which can move a norm across a rounding tie; everything behind the norms is then exact."""
import math

import numpy as np

SEG_DECAY = 1
SEG_ADAPT = 2


def ref_segment_norms(x, bounds):
    """norm[s] = (float)sqrt(sum over the segment of (double)x[i]^2)"""
    x = np.asarray(x, np.float32)
    return np.array([np.float32(np.sqrt(np.sum(x[int(b):int(e)].astype(np.float64) ** 2))) for b, e in zip(bounds[:-1], bounds[1:])],
                    np.float32)


def _per_element(values, bounds, n):
    """a per-segment array spread over the elements"""
    bounds = np.asarray(bounds, np.int64)
    assert bounds[0] == 0 and bounds[-1] == n and np.all(np.diff(bounds) > 0)
    return np.repeat(np.asarray(values), np.diff(bounds))


def lamb_host_scalars(step, beta1, beta2):
    """(omb1, omb2, bc2s, bc1) as the entry point computes them"""
    f = np.float32
    beta1, beta2 = f(beta1), f(beta2)
    omb1 = f(f(1) - beta1)
    omb2 = f(f(1) - beta2)
    bc2s = f(math.sqrt(1.0 - math.pow(float(beta2), float(int(step)))))
    bc1 = f(1.0 - math.pow(float(beta1), float(int(step))))
    return omb1, omb2, bc2s, bc1


def ref_lamb_moments(p, g, m, v, bounds, flags, step, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, grad_scale=1.0):
    """the first pass -> (r, m', v'):
        gs = g * grad_scale (only when grad_scale != 1);  m' = beta1 * m + omb1 * gs;  v' = beta2 * v + omb2 * (gs * gs)
        den = sqrt(v') / bc2s + eps;  mh = m' / bc1;  q = mh / den;  r = q + weight_decay * p (DECAY segments, weight_decay != 0) or q"""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    assert p.ndim == 1 and p.shape == g.shape == m.shape == v.shape and int(step) >= 1
    omb1, omb2, bc2s, bc1 = lamb_host_scalars(step, beta1, beta2)
    beta1, beta2, eps, weight_decay, grad_scale = f(beta1), f(beta2), f(eps), f(weight_decay), f(grad_scale)
    gs = g * grad_scale if grad_scale != f(1) else g
    with np.errstate(all="ignore"):
        b1m = beta1 * m
        o1g = omb1 * gs
        m_new = b1m + o1g
        b2v = beta2 * v
        gg = gs * gs
        o2g = omb2 * gg
        v_new = b2v + o2g
        root = np.sqrt(v_new)
        rb = root / bc2s
        den = rb + eps
        mh = m_new / bc1
        q = mh / den
        r = q.copy()
        if weight_decay != f(0):
            mask = _per_element((np.asarray(flags) & SEG_DECAY) != 0, bounds, p.size)
            wp = weight_decay * p
            r[mask] = (q + wp)[mask]
    for a in (gs, b1m, o1g, m_new, b2v, gg, o2g, v_new, root, rb, den, mh, q, r):
        assert a.dtype == f
    return r, m_new, v_new


def ref_lamb_ratio(w_norm, u_norm, flags):
    """ratio[s] = w_norm / u_norm where ADAPT is set and both norms are positive, exactly 1 elsewhere"""
    f = np.float32
    w, u = np.asarray(w_norm, f), np.asarray(u_norm, f)
    use = ((np.asarray(flags) & SEG_ADAPT) != 0) & (w > 0) & (u > 0)
    with np.errstate(all="ignore"):
        q = w / u
    out = np.where(use, q, f(1)).astype(f)
    return out


def ref_lamb_step(p, g, m, v, bounds, flags, step, lr, w_norm, u_norm, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, grad_scale=1.0):
    """one LAMB step over flat fp32 arrays from GIVEN norms (w_norm of p, u_norm of r, per segment) -> (p', m', v', r, ratio):
        t = ratio[s] * r;  p' = p - lr * t"""
    f = np.float32
    p = np.asarray(p, f)
    r, m_new, v_new = ref_lamb_moments(p, g, m, v, bounds, flags, step, beta1, beta2, eps, weight_decay, grad_scale)
    ratio = ref_lamb_ratio(w_norm, u_norm, flags)
    with np.errstate(all="ignore"):
        t = _per_element(ratio, bounds, p.size) * r
        stp = f(lr) * t
        p_new = p - stp
    for a in (t, stp, p_new):
        assert a.dtype == f
    return p_new, m_new, v_new, r, ratio


def ref_lars_ratio(w_norm, g_norm, flags, weight_decay, trust_coefficient=1e-3, eps=1e-8, grad_scale=1.0):
    """-> (gnt, ratio):  gnt = g_norm * grad_scale (only when grad_scale != 1);  wds = weight_decay on DECAY segments, 0 elsewhere;
    ratio[s] = (trust_coefficient * w_norm) / ((gnt + wds * w_norm) + eps) where ADAPT is set and w_norm, gnt > 0, exactly 1 elsewhere.
    Starting from the device's own u_norm -- which has grad_scale folded in already -- pass grad_scale = 1."""
    f = np.float32
    w, gn = np.asarray(w_norm, f), np.asarray(g_norm, f)
    flags = np.asarray(flags)
    grad_scale = f(grad_scale)
    with np.errstate(all="ignore"):
        gnt = gn * grad_scale if grad_scale != f(1) else gn
        wds = np.where((flags & SEG_DECAY) != 0, f(weight_decay), f(0)).astype(f)
        num = f(trust_coefficient) * w
        ww = wds * w
        s1 = gnt + ww
        den = s1 + f(eps)
        q = num / den
    for a in (gnt, num, ww, s1, den, q):
        assert a.dtype == f
    use = ((flags & SEG_ADAPT) != 0) & (w > 0) & (gnt > 0)
    return gnt, np.where(use, q, f(1)).astype(f)


def ref_lars_step(p, g, v, bounds, flags, lr, w_norm, g_norm, momentum=0.0, weight_decay=0.0, trust_coefficient=1e-3, eps=1e-8, nesterov=False,
                  grad_scale=1.0, norm_is_scaled=False):
    """one LARS step over flat fp32 arrays from GIVEN norms (w_norm of p, g_norm of the unscaled g, per segment; norm_is_scaled: g_norm
    is the device's u_norm, grad_scale folded in already) -> (p', v', gnt, ratio):
        gs = g * grad_scale (only when grad_scale != 1);  d = gs + weight_decay * p (DECAY segments, weight_decay != 0) or gs
        dl = ratio[s] * d;  momentum == 0: u = dl (v comes back untouched);  otherwise v' = momentum * v + dl, u = dl + momentum * v'
        (nesterov) or v';  p' = p - lr * u"""
    f = np.float32
    p, g = np.asarray(p, f), np.asarray(g, f)
    assert p.ndim == 1 and p.shape == g.shape
    gnt, ratio = ref_lars_ratio(w_norm, g_norm, flags, weight_decay, trust_coefficient, eps, 1.0 if norm_is_scaled else grad_scale)
    lr, momentum, weight_decay, grad_scale = f(lr), f(momentum), f(weight_decay), f(grad_scale)
    with np.errstate(all="ignore"):
        gs = g * grad_scale if grad_scale != f(1) else g
        d = gs.copy()
        if weight_decay != f(0):
            mask = _per_element((np.asarray(flags) & SEG_DECAY) != 0, bounds, p.size)
            wp = weight_decay * p
            d[mask] = (gs + wp)[mask]
        dl = _per_element(ratio, bounds, p.size) * d
        if momentum == f(0):
            u, v_new = dl, v
        else:
            v = np.asarray(v, f)
            assert v.shape == p.shape
            mv = momentum * v
            v_new = mv + dl
            if nesterov:
                mvn = momentum * v_new
                u = dl + mvn
            else:
                u = v_new
        stp = lr * u
        p_new = p - stp
    for a in (gs, d, dl, u, stp, p_new):
        assert a.dtype == f
    return p_new, v_new, gnt, ratio


def segment_table_of(layout, decay_bias_and_norm=False, adapt_bias_and_norm=False):
    """(bounds, flags) of a cnn_amd.stacks.walk() layout in arena (= checkpoint) order, as Sequential::set_lamb / set_lars build them:
    Conv2D / LinearLayer: weights, bias;  BatchNorm2D: gamma, beta, moving_mean, moving_var.  Weights get DECAY | ADAPT; biases and
    gamma / beta get DECAY / ADAPT only with the matching *_bias_and_norm flag; moving statistics get neither."""
    bounds, flags, off = [0], [], 0
    small = (SEG_DECAY if decay_bias_and_norm else 0) | (SEG_ADAPT if adapt_bias_and_norm else 0)
    for e in layout:
        n = e["params"]
        if n == 0:
            continue
        if e["kind"] in ("conv", "linear"):
            nb = e["Co"] if e["kind"] == "conv" else e["n_out"]
            parts = [(n - nb, SEG_DECAY | SEG_ADAPT), (nb, small)]
        elif e["kind"] == "bn":
            c = n // 4
            parts = [(c, small), (c, small), (c, 0), (c, 0)]
        else:
            raise AssertionError(f"segment_table_of: a {e['kind']} layer with parameters")
        for cnt, fl in parts:
            off += cnt
            bounds.append(off)
            flags.append(fl)
    return np.array(bounds, np.uint32), np.array(flags, np.uint32)
