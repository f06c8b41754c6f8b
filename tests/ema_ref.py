"""Host reference of the parameter average (cnn_ema_decay_at, cnn_ema_update, include/cnn_amd.h).  NumPy only; every intermediate is an
np.float32 array, so every product and sum is rounded separately -- the arithmetic the kernel is held to bit for bit."""
import numpy as np


def ref_ema_decay_at(decay, warmup, t):
    """the decay of the update that follows t earlier ones: decay, or with warmup min(decay, (float)((1.0 + t) / (10.0 + t)))"""
    f = np.float32
    decay = f(decay)
    if not warmup:
        return decay
    t = float(int(t))  # (double)uint64
    ramp = f((1.0 + t) / (10.0 + t))
    return ramp if ramp < decay else decay


def ref_ema_update(ema, p, decay, ranges):
    """one update over flat fp32 arrays -> ema'.  ranges: [(begin, end)] half-open index ranges that are averaged.
        decay == 0        : ema' = p                          (a copy of the bits; ema is not looked at)
        inside a range    : ema' = decay * ema + omd * p      (omd = 1.f - decay; two products, one sum)
        elsewhere         : ema' = p                          (a copy of the bits)"""
    f = np.float32
    p = np.asarray(p, f)
    assert p.ndim == 1
    decay = f(decay)
    out = p.copy()
    if decay == f(0):
        return out
    ema = np.asarray(ema, f)
    assert ema.shape == p.shape
    omd = f(1) - decay
    mask = np.zeros(p.size, bool)
    for b, e in ranges:
        mask[int(b):int(e)] = True
    with np.errstate(all="ignore"):
        de = decay * ema
        op = omd * p
        s = de + op
    assert de.dtype == f and op.dtype == f and s.dtype == f and type(omd) is f
    out.view(np.uint32)[mask] = s.view(np.uint32)[mask]
    return out


def merged(ranges):
    """adjacent ranges merged, as the container's table"""
    out = []
    for b, e in ranges:
        if out and out[-1][1] == b:
            out[-1] = (out[-1][0], e)
        else:
            out.append((b, e))
    return out
