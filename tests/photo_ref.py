"""The photometric epilogue of the photo stager's kernel (include/cnn_amd.h, cnn_batch_stager_create_u8_photo) restated in NumPy behind
tests/augment_ref.py's gather rule: float32 arrays, one rounding per operation -- the kernel must equal this bit for bit.  Sample b has 20
floats p[b][0..19]; the stager has s[3], t[3] and a clamp flag.  Per output pixel (x, y):

    v0,v1,v2 = the gather rule's three channel values of this pixel (inside pixels only)
    u_c   = ((A[c][0]*v0 + A[c][1]*v1) + A[c][2]*v2) + o[c]        A = p[0..8] row-major, o = p[9..11]
    u_c   = clamp ? fminf(fmaxf(u_c, 0), 1) : u_c                   (np.fmin / np.fmax)
    out_c = u_c * s[c] + t[c]                                      (normalisation: s = 1/std, t = -mean/std)
    out_c = inside ? out_c : fill                                  (fill is in OUTPUT units: the colour stage does not touch it)
    ex0,ey0,ew,eh = p[12..15] (whole numbers), ev[c] = p[16..18], p[19] reserved = 0
    out_c = (ex0 <= x && x < ex0+ew && ey0 <= y && y < ey0+eh) ? ev[c] : out_c     (fp32 comparisons; ev in output units)

The identity: with A = I, o = 0, clamp off, s = 1, t = 0 and no box (ew == 0 or eh == 0) -- IDENTITY below, what acquire() presets -- the
rule returns the gather rule's bits unchanged.  The table values and their blends are finite, so 1*v + 0*w == v, v + 0 == v and
v*1 + 0 == v (a -0 could only become +0, which compares equal); photo() asserts nothing about it, tests/test_gpu_photo.py holds it on
the reference and on the device.

A plain module: the tests import it (`from tests import photo_ref`)."""
import numpy as np

from tests import augment_ref

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], dtype=F)


def normalize_consts(mean, std):
    """cnn_batch_stager_set_normalize: s = 1/std, t = -mean/std from the fp32 arguments, in double, rounded once"""
    mean, std = np.asarray(mean, dtype=F).astype(np.float64), np.asarray(std, dtype=F).astype(np.float64)
    return (1.0 / std).astype(F), (-mean / std + 0.0).astype(F)


def photo(src_u8, matrices, params, H, W, fill=0.0, s=(1, 1, 1), t=(0, 0, 0), clamp=False):
    """-> (fp32 [B][3][H][W], bool [B][H][W] `inside` of the gather rule, bool [B][H][W] `box`, fp32 [B][3][H][W] u before the clamp)"""
    geo, inside = augment_ref.augment(src_u8, matrices, H, W, fill)
    p = np.asarray(params, dtype=F)
    B = geo.shape[0]
    assert p.shape == (B, 20)
    s, t = np.asarray(s, dtype=F), np.asarray(t, dtype=F)
    out = np.empty_like(geo)
    raw = np.empty_like(geo)
    box_all = np.empty((B, H, W), dtype=bool)
    x = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    with np.errstate(all="ignore"):
        for b in range(B):
            v0, v1, v2 = geo[b, 0], geo[b, 1], geo[b, 2]
            ex0, ey0, ew, eh = (F(v) for v in p[b, 12:16])
            box = (x >= ex0) & (x < F(ex0 + ew)) & (y >= ey0) & (y < F(ey0 + eh))
            for c in range(3):
                a0, a1, a2, o = (F(v) for v in (p[b, 3 * c], p[b, 3 * c + 1], p[b, 3 * c + 2], p[b, 9 + c]))
                u = (((a0 * v0).astype(F) + (a1 * v1).astype(F)).astype(F) + (a2 * v2).astype(F)).astype(F) + o
                assert u.dtype == F
                raw[b, c] = u
                if clamp:
                    u = np.fmin(np.fmax(u, F(0)), F(1))
                val = ((u * s[c]).astype(F) + t[c]).astype(F)
                val = np.where(inside[b], val, F(fill))
                out[b, c] = np.where(box, p[b, 16 + c], val)
            box_all[b] = box
    return out, inside, box_all, raw
