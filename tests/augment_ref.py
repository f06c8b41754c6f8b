"""The rule of cnn_augment_u8 (include/cnn_amd.h) restated in NumPy: float32 arrays, one rounding per operation -- the kernel must equal
this bit for bit.  Input: interleaved bytes [B][Hs][Ws][3]; output: planar fp32 [B][3][H][W]; m[b][0..5] maps output pixel indices to
source pixel indices.  Per output pixel (x, y):

    sx = (m0*x + m1*y) + m2            sy = (m3*x + m4*y) + m5
    inside = sx >= -0.5f && sx <= Ws-0.5f && sy >= -0.5f && sy <= Hs-0.5f
    x0f = floorf(sx); fx = sx - x0f;   y0f = floorf(sy); fy = sy - y0f
    x0 = clamp((int)x0f, 0, Ws-1); x1 = clamp((int)x0f + 1, 0, Ws-1)      (same for y)
    t.. = lut[byte]                    (lut[v] = v * 1.f / 255)
    top = t00 + fx*(t01 - t00); bot = t10 + fx*(t11 - t10); out = top + fy*(bot - top)
    out = inside ? out : fill

A plain module: the tests import it (`from tests import augment_ref`)."""
import numpy as np

F = np.float32
LUT = (np.arange(256).astype(F) * F(1.0) / F(255)).astype(F)  # Tensor3D::read_from_opencv_mat's expression, data_format.cpp:19-21


def plain(src_u8):
    """the plain conversion: bytes [B][Hs][Ws][3] -> fp32 [B][3][Hs][Ws]"""
    return np.ascontiguousarray(LUT[src_u8].transpose(0, 3, 1, 2))


def augment(src_u8, matrices, H, W, fill=0.0):
    """-> (fp32 [B][3][H][W], bool [B][H][W] `inside`)"""
    src_u8 = np.asarray(src_u8)
    m = np.asarray(matrices, dtype=F)
    B, Hs, Ws, ch = src_u8.shape
    assert ch == 3 and src_u8.dtype == np.uint8 and m.shape == (B, 6)
    out = np.empty((B, 3, H, W), dtype=F)
    inside_all = np.empty((B, H, W), dtype=bool)
    x = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    with np.errstate(all="ignore"):
        for b in range(B):
            m0, m1, m2, m3, m4, m5 = (F(v) for v in m[b])
            sx = ((m0 * x).astype(F) + (m1 * y).astype(F)).astype(F) + m2
            sy = ((m3 * x).astype(F) + (m4 * y).astype(F)).astype(F) + m5
            assert sx.dtype == F and sy.dtype == F
            inside = (sx >= F(-0.5)) & (sx <= F(Ws) - F(0.5)) & (sy >= F(-0.5)) & (sy <= F(Hs) - F(0.5))
            x0f, y0f = np.floor(sx), np.floor(sy)
            fx, fy = (sx - x0f).astype(F), (sy - y0f).astype(F)
            xi = np.where(inside, x0f, F(0)).astype(np.int64)  # (the integer is only taken where it is in range: -1 .. Ws-1)
            yi = np.where(inside, y0f, F(0)).astype(np.int64)
            x0, x1 = np.clip(xi, 0, Ws - 1), np.clip(xi + 1, 0, Ws - 1)
            y0, y1 = np.clip(yi, 0, Hs - 1), np.clip(yi + 1, 0, Hs - 1)
            img = LUT[src_u8[b]]  # [Hs][Ws][3] fp32
            for c in range(3):
                p = img[:, :, c]
                t00, t01, t10, t11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
                top = (t00 + (fx * (t01 - t00).astype(F)).astype(F)).astype(F)
                bot = (t10 + (fx * (t11 - t10).astype(F)).astype(F)).astype(F)
                val = (top + (fy * (bot - top).astype(F)).astype(F)).astype(F)
                out[b, c] = np.where(inside, val, F(fill))
            inside_all[b] = inside
    return out, inside_all
