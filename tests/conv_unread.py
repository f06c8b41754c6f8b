"""The dead elements of a convolution input: positions of x that no window of (H, W, k, s, pad) covers.

The reference never reads them (conv2d.cpp:127-146: the window loops stop at the last full window) and zero-fills their gradient
(conv2d.cpp:168).  With stride > 1 the last rows / columns can be dead (224 x 224, k 3, s 2: row and column 223), with k < s a whole
lattice is (1 x 1, stride 2).  Pure NumPy; tests/test_conv_unread.py holds it against an enumeration of all windows."""
import numpy as np


def _covered(n, k, s, pad):
    """bool[n]: position i of one axis lies in some window [o * s - pad, o * s - pad + k), o < (n + 2 pad - k) // s + 1"""
    n_out = (n + 2 * pad - k) // s + 1
    p = np.arange(n) + pad                     # position in the padded axis
    o = np.minimum(p // s, n_out - 1)          # the last window that starts at or before p
    return (n_out > 0) & (p - o * s < k)


def unread_mask(case):
    """case = (B, Ci, H, W, Co, k, s, pad[, flags]) -> bool[H, W], True where no window covers x[:, :, h, w]"""
    H, W, k, s, pad = case[2], case[3], case[5], case[6], case[7]
    return ~np.outer(_covered(H, k, s, pad), _covered(W, k, s, pad))


def poisoned(x, mask, word):
    """a copy of x (B, C, H, W fp32) with the 32-bit pattern `word` at the dead positions"""
    out = np.array(x, np.float32, copy=True)
    out.view(np.uint32)[:, :, mask] = np.uint32(word)
    return out
