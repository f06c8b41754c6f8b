"""The half-size levels of the resident dataset (include/cnn_amd.h, cnn_dataset_create_u8_levels) restated in NumPy, in three parts:

    halve(img)                the edge-replicated 2 x 2 box, rounded half up, in integers: one level from the level before it
    choose(m, L)              the level a map picks out of L levels and the map on that level, in Python floats (doubles)
    resident_levels(...)      the chain per image, the choice per sample, then tests/resident_ref.py (imported, unchanged) on the level's
                              images with the level's map

A plain module: the tests import it (`from tests import mip_ref`)."""
import math

import numpy as np

from tests import resident_ref

F = np.float32


def halve(img):
    """uint8 [..., H, W, 3] -> uint8 [..., (H + 1) // 2, (W + 1) // 2, 3]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim >= 3 and img.shape[-1] == 3
    Hp, Wp = img.shape[-3], img.shape[-2]
    H, W = (Hp + 1) // 2, (Wp + 1) // 2
    y0, x0 = 2 * np.arange(H), 2 * np.arange(W)
    y1, x1 = np.minimum(y0 + 1, Hp - 1), np.minimum(x0 + 1, Wp - 1)
    p = img.astype(np.int64)
    rows0, rows1 = p[..., y0, :, :], p[..., y1, :, :]
    v = rows0[..., x0, :] + rows0[..., x1, :] + rows1[..., x0, :] + rows1[..., x1, :] + 2
    return (v >> 2).astype(np.uint8)


def chain(img, L):
    """-> [level 0, ..., level L - 1] of uint8 [..., H, W, 3]"""
    out = [np.asarray(img)]
    for _ in range(1, L):
        assert out[-1].shape[-3] > 1 or out[-1].shape[-2] > 1, "more levels than the size has"
        out.append(halve(out[-1]))
    return out


def max_levels(Hs, Ws):
    n = 1
    while Hs > 1 or Ws > 1:
        Hs, Ws, n = (Hs + 1) // 2, (Ws + 1) // 2, n + 1
    return n


def choose(m, L):
    """-> (level, float32 (6,) map on that level) for the six fp32 floats m and a dataset of L levels"""
    m = np.asarray(m, dtype=F).reshape(6)
    m0, m1, m2, m3, m4, m5 = (float(v) for v in m)
    rx, ry = math.sqrt(m0 * m0 + m3 * m3), math.sqrt(m1 * m1 + m4 * m4)  # (a NaN or an infinity passes through: no level above 0)
    level = 0
    if math.isfinite(rx) and math.isfinite(ry):
        r = max(rx, ry)
        while level + 1 < L and r >= float(2 ** (level + 1)):
            level += 1
    if level == 0:
        return 0, m.copy()
    k = float(2 ** level)
    with np.errstate(all="ignore"):
        out = np.array([F(m0 / k), F(m1 / k), F((m2 + 0.5) / k - 0.5), F(m3 / k), F(m4 / k), F((m5 + 0.5) / k - 0.5)], dtype=F)
    return level, out


def resident_levels(images_u8, labels, indices, matrices, params, H, W, L, fill=0.0, s=(1, 1, 1), t=(0, 0, 0), clamp=False):
    """-> (fp32 [B][3][H][W], int32 [B] labels, int32 [B] levels) of the gather of `indices` out of a dataset of L levels"""
    levels_of = chain(images_u8, L)
    idx = np.asarray(indices, dtype=np.int64)
    mats, params = np.asarray(matrices, dtype=F).reshape(-1, 6), np.asarray(params, dtype=F)
    B = idx.shape[0]
    out, lab, lev = np.empty((B, 3, H, W), F), np.empty(B, np.int32), np.empty(B, np.int32)
    for b in range(B):
        lev[b], mb = choose(mats[b], L)
        o, l = resident_ref.resident(levels_of[lev[b]], labels, idx[b:b + 1], mb[None, :], params[b:b + 1], H, W, fill, s, t, clamp)
        out[b], lab[b] = o[0], l[0]
    return out, lab, lev
