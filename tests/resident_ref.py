"""The rule of the resident stager's kernel (include/cnn_amd.h, cnn_batch_stager_create_u8_resident) restated in NumPy: tests/photo_ref.py
behind tests/augment_ref.py (both imported, unchanged) applied to images[idx].  Sample b reads idx = indices[b]:

    source  = images[idx]                              (sample idx of the dataset's store)
    idx == -1: no pixel of the sample is inside, no byte of the store is read: every pixel is `fill`, an erase box still applies
    label_b = idx < 0 ? -1 : labels[idx]

A plain module: the tests import it (`from tests import resident_ref`)."""
import numpy as np

from tests import photo_ref

F = np.float32


def identity_params(B, Hs, Ws, H, W):
    """what acquire() presets for equal sizes: the identity map and the identity photo block ((B, 6), (B, 20)); other sizes take the
    plain resize map from capi.augment_matrix([], Hs, Ws, H, W)"""
    assert (Hs, Ws) == (H, W)
    return np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=F), (B, 1)), np.tile(photo_ref.IDENTITY, (B, 1))


def resident(images_u8, labels, indices, matrices, params, H, W, fill=0.0, s=(1, 1, 1), t=(0, 0, 0), clamp=False):
    """-> (fp32 [B][3][H][W], int32 [B] labels) of the gather of `indices` out of the dataset (images_u8 [N][Hs][Ws][3], labels [N])"""
    images_u8, labels, idx = np.asarray(images_u8), np.asarray(labels, dtype=np.int32), np.asarray(indices, dtype=np.int64)
    N = images_u8.shape[0]
    assert idx.ndim == 1 and ((idx >= -1) & (idx < N)).all() and labels.shape == (N,)
    present = idx >= 0
    src = images_u8[np.where(present, idx, 0)]  # (an absent row's bytes are never looked at: see below)
    out, inside, box, _ = photo_ref.photo(src, matrices, params, H, W, fill, s, t, clamp)
    p = np.asarray(params, dtype=F)
    for b in np.flatnonzero(~present):  # "no pixel inside": fill, then the box
        for c in range(3):
            out[b, c] = np.where(box[b], p[b, 16 + c], F(fill))
    return out, np.where(present, labels[np.where(present, idx, 0)], -1).astype(np.int32)
