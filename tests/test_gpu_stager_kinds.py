"""Every kind of batch stager end to end at the smallest shapes (include/cnn_amd.h: cnn_batch_stager_create, _create_u8, _create_u8_aug,
_create_u8_photo, _create_u8_resident on a one-level and on a levelled dataset), through cnn_amd.capi.  B = 3 (odd: no part of a slot's
parameter block is 16-byte aligned by accident), depth = 2 and three rounds of acquire / fill / submit / wait / release, so that slot 0
is used twice and its `consumed` event is waited for.  Sources are 8 x 8; the outputs 8 x 8 (16-byte stores) and 5 x 3 (per-pixel
stores); the levelled dataset has four levels, the last of them 1 x 1 (three bytes: the byte-load route).  Every sample of every round has
its own map, photo block and index, one index per round is -1.  Every round's batch -- for the resident kinds also its labels and
levels -- equals, bit for bit, what tests/augment_ref.py, photo_ref.py, resident_ref.py and mip_ref.py give (raw: the bytes as they
are; u8: the plain conversion), and every accessor works on exactly the kinds that have its part and raises its message on the others.

The file pins the stagers' behaviour as it was before they moved into cnn_amd/csrc/staging.hip: it passes against the library built from
the commit before that move (CNN_AMD_LIB=<that build>/libcnn_amd.so) and against this tree's."""
import ctypes as C

import numpy as np
import pytest

from tests import augment_ref as R
from tests import mip_ref as M
from tests import photo_ref as P
from tests import resident_ref as RR

pytestmark = pytest.mark.gpu

F = np.float32
B, DEPTH, ROUNDS = 3, 2, 3
HS = WS = 8
N, LEVELS = 4, 4
FILL = -0.5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
KINDS = ["raw", "u8", "aug", "photo", "resident", "resident_levels"]
OUTS = [(8, 8), (5, 3)]
INDICES = np.array([[2, 0, -1], [1, -1, 3], [-1, 3, 0]], np.int32)  # per round: each sample is absent once
# accessor -> the kinds that have it; the message of the others
HAS = {"matrices": KINDS[2:], "set_fill": KINDS[2:], "photo": KINDS[3:], "set_normalize": KINDS[3:], "indices": KINDS[4:], "labels": KINDS[4:],
       "levels": KINDS[5:]}
LACKS = {"matrices": "not an augmenting stager", "set_fill": "not an augmenting stager", "photo": "not a photo stager",
         "set_normalize": "not a photo stager", "indices": "not a resident stager", "labels": "not a resident stager"}


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture(scope="module")
def store():
    """what the two datasets hold: N images of 8 x 8 and their labels"""
    images = np.random.RandomState(7).randint(0, 256, size=(N, HS, WS, 3)).astype(np.uint8)
    return images, np.arange(20, 20 + N, dtype=np.int32)


def maps(kind, r):
    """(B, 6): a mirror, a half-pixel shift (four taps) and a rotation; round r shifts each by r whole source pixels.  For the levelled
    dataset: scales of 1, 2 and 8, which land on levels 0, 1 and 3"""
    from cnn_amd import capi

    if kind == "resident_levels":
        m = np.array([[-1, 0, WS - 1, 0, 1, 0], [2, 0, 0.5, 0, 2, 0.5], [8, 0, 3.5, 0, 8, 3.5]], F)
    else:
        m = np.array([[-1, 0, WS - 1, 0, 1, 0], [1, 0, 0.5, 0, 1, 0.5], capi.augment_matrix([(capi.AUG_ROTATE, 30.0)], HS, WS, HS, WS)], F)
    m[:, 2] += F(r)
    return m


def photo_blocks(r):
    """(B, 20): a colour map and an erase box per sample, the box's edges cutting a quad of four output pixels"""
    from cnn_amd import capi

    blocks = np.tile(P.IDENTITY, (B, 1))
    for b in range(B):
        blocks[b, :12] = capi.colour_matrix([(capi.COL_BRIGHTNESS, 1.3 - 0.1 * b), (capi.COL_CONTRAST, 1.6, 0.5), (capi.COL_SATURATION, 0.5 + 0.2 * r),
                                             (capi.COL_HUE, 15.0 * (b + 1))])
        blocks[b, 12:19] = (1 + b, r, 2, 2, 10.0 + b, 20.0 + r, 30.0 + b)
    return blocks


def copy_out(T, dev, shape, dtype=None):
    """the device buffer behind `dev` as a NumPy array, copied on the current stream (behind the stager's wait())"""
    from cnn_amd import capi

    got = T.empty(shape, dtype=dtype or T.float32, device="cuda")
    capi.check(capi.load().cnn_memcpy_d2d(got.data_ptr(), C.c_void_p(dev), got.numel() * 4, capi._stream()), "cnn_memcpy_d2d")
    return got


def check_accessors(capi, kind, st, slot):
    """every accessor either works or raises its message; the working setters are left at the values the rounds run with"""
    st.B = B  # (the raw and the u8 wrapper keep no batch size; the views below need one only where the call succeeds)
    calls = {"matrices": lambda: st.matrices(slot), "set_fill": lambda: st.set_fill(FILL), "photo": lambda: st.photo(slot),
             "set_normalize": lambda: st.set_normalize(MEAN, STD, True), "indices": lambda: st.indices(slot), "labels": lambda: st.labels(slot),
             "levels": lambda: st.levels(slot)}
    for name, call in calls.items():
        if kind in HAS[name]:
            call()
        else:
            message = "one level" if (name, kind) == ("levels", "resident") else LACKS.get(name, "not a resident stager")
            with pytest.raises(capi.CnnAmdError, match=message):
                call()


@pytest.mark.parametrize("H, W", OUTS, ids=["quad_8x8", "px_5x3"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_rounds(T, store, kind, H, W):
    from cnn_amd import capi

    images, labels = store
    s, t = P.normalize_consts(MEAN, STD)
    ds = None
    if kind in ("resident", "resident_levels"):
        ds = capi.ResidentDataset(N, HS, WS, levels=LEVELS if kind == "resident_levels" else 1)
        ds.write(0, images, labels)
        if kind == "resident_levels":
            assert ds.level_shape(LEVELS - 1) == (1, 1)
        st = capi.BatchStager(u8_shape=(B, H, W), resident=ds, depth=DEPTH)
    elif kind == "raw":
        st = capi.BatchStager(B * 3 * H * W * 4, depth=DEPTH)
    elif kind == "u8":
        st = capi.BatchStager(u8_shape=(B, H, W), depth=DEPTH)
    else:
        st = capi.BatchStager(u8_shape=(B, H, W), source_shape=(HS, WS), photo=kind == "photo", depth=DEPTH)
    try:
        slots = []
        for r in range(ROUNDS):
            rs = np.random.RandomState(100 + r)
            host, slot = st.acquire()
            slots.append(slot)
            if r == 0:
                check_accessors(capi, kind, st, slot)
            want_lab = want_lev = None
            if kind == "raw":
                src = rs.standard_normal(B * 3 * H * W).astype(F)
                host[:] = src
                want = src.reshape(B, 3, H, W)
            elif kind == "u8":
                src = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
                host[:] = src.reshape(-1)
                want = R.plain(src)
            else:
                m, blocks, idx = maps(kind, r), photo_blocks(r), INDICES[r]
                if ds is None:
                    src = rs.randint(0, 256, size=(B, HS, WS, 3)).astype(np.uint8)
                    host[:] = src.reshape(-1)
                else:
                    assert host is None
                    assert st.indices(slot).tolist() == [-1] * B, "acquire() presets the indices"
                    st.indices(slot)[:] = idx
                assert st.matrices(slot).tobytes() == np.tile(capi.augment_matrix([], HS, WS, H, W), (B, 1)).tobytes(), "acquire() presets the maps"
                st.matrices(slot)[:] = m
                if kind == "aug":
                    want = R.augment(src, m, H, W, FILL)[0]
                else:
                    assert st.photo(slot).tobytes() == np.tile(P.IDENTITY, (B, 1)).tobytes(), "acquire() presets the photo blocks"
                    st.photo(slot)[:] = blocks
                    if kind == "photo":
                        want = P.photo(src, m, blocks, H, W, FILL, s, t, True)[0]
                    elif kind == "resident":
                        want, want_lab = RR.resident(images, labels, idx, m, blocks, H, W, FILL, s, t, True)
                    else:
                        want, want_lab, want_lev = M.resident_levels(images, labels, idx, m, blocks, H, W, LEVELS, FILL, s, t, True)
                        assert want_lev.tolist() == [0, 1, 3]
            dev = st.submit(slot)
            st.wait(slot)
            got = copy_out(T, dev, (B, 3, H, W))
            lab = copy_out(T, st.labels(slot), (B,), T.int32) if ds is not None else None
            st.release(slot)
            T.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == np.ascontiguousarray(want, F).tobytes(), (kind, r)
            if ds is not None:
                assert np.array_equal(lab.cpu().numpy(), want_lab) and (want_lab == -1).sum() == 1, (kind, r)
                assert st.matrices(slot).tobytes() == m.tobytes(), "submit() leaves the caller's maps as they are"
            if want_lev is not None:
                assert np.array_equal(st.levels(slot), want_lev), (kind, r)
        assert slots == [0, 1, 0]
        if ds is not None:
            with pytest.raises(capi.CnnAmdError, match="still attached"):
                ds.close()
    finally:
        st.close()
        if ds is not None:
            ds.close()  # the closed stager has left it destroyable
            assert ds.h is None
