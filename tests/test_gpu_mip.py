"""The half-size levels of the device-resident dataset (include/cnn_amd.h: cnn_dataset_create_u8_levels, _read_level, _level_info,
cnn_batch_stager_levels) on the device, through cnn_amd.capi.  Every comparison is bit for bit against tests/mip_ref.py: halve() for
the levels that cnn_dataset_write builds, choose() for the level a map picks, resident_levels() for the gather.  The batch helpers
(acquire -> indices / parameters -> submit -> wait -> copy out -> release) are those of tests/test_gpu_resident.py.  The shapes are the
smallest at which each thing can go wrong: odd sizes whose last row and column are the replicated edge, levels of 18 and 6 bytes (the
pulled-back 8-byte load and the byte-load route), a batch whose samples sit on four different levels, and one store whose second level
crosses byte 2^32."""
import numpy as np
import pytest

from tests import augment_ref as R
from tests import mip_ref as M
from tests import photo_ref as P
from tests import test_gpu_resident as RG

pytestmark = pytest.mark.gpu

F = np.float32
FILL = -1.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUTS = [(4, 8), (3, 5)]


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def make_dataset(n, Hs, Ws, L, seed):
    from cnn_amd import capi

    images = np.random.RandomState(seed).randint(0, 256, size=(n, Hs, Ws, 3)).astype(np.uint8)
    labels = np.arange(10, 10 + n, dtype=np.int32)
    ds = capi.ResidentDataset(n, Hs, Ws, levels=L)
    ds.write(0, images, labels)
    return ds, images, labels


def level_shift_map(l, Hl, Wl, H, W):
    """the level-0 map that lands on level l as a half-pixel shift whose LAST output pixel samples (Wl - 0.5, Hl - 0.5): four taps, the
    last of them the level's last pixel, so a pulled-back load ends with the sample.  Every value is exact in fp32"""
    k = float(2 ** l)
    m = np.array([k, 0, (((Wl - 0.5) - (W - 1)) + 0.5) * k - 0.5, 0, k, (((Hl - 0.5) - (H - 1)) + 0.5) * k - 0.5], F)
    level, on_level = M.choose(m, l + 1)
    assert level == l and on_level.tolist() == [1, 0, (Wl - 0.5) - (W - 1), 0, 1, (Hl - 0.5) - (H - 1)]
    return m


# ---- 1. the levels that write() builds -------------------------------------------------------------------------------------------------
SIZES = [(5, 7, 4), (1, 1, 1), (1, 9, 5), (8, 8, 4), (33, 17, 7)]


@pytest.mark.parametrize("Hs, Ws, L", SIZES, ids=[f"{h}x{w}_L{l}" for h, w, l in SIZES])
def test_levels_after_write(T, Hs, Ws, L):
    from cnn_amd import capi

    n = 5
    assert L == M.max_levels(Hs, Ws) == capi.dataset_max_levels(Hs, Ws)
    if (Hs, Ws) == (5, 7):
        assert [lv.shape for lv in M.chain(np.zeros((Hs, Ws, 3), np.uint8), L)] == [(5, 7, 3), (3, 4, 3), (2, 2, 3), (1, 1, 3)]
    rs = np.random.RandomState(1000 + Hs)
    images = rs.randint(0, 256, size=(n, Hs, Ws, 3)).astype(np.uint8)
    ds = capi.ResidentDataset(n, Hs, Ws, levels=L)
    try:
        assert ds.levels == L and ds.info() == (n, Hs, Ws)
        for l, lv in enumerate(M.chain(images, L)):
            assert ds.level_shape(l) == lv.shape[1:3]
            assert not ds.read_level(l, 0, n).any(), "a fresh dataset reads zeros at every level"
        _, counts = RG.logged(capi, T, lambda: ds.write(0, images, np.arange(n)))
        assert counts == ({"dataset_halve_u8": L - 1} if L > 1 else {}), counts
        for l, lv in enumerate(M.chain(images, L)):
            assert np.array_equal(ds.read_level(l, 0, n), lv), l
        assert np.array_equal(ds.read(0, n)[0], images)
        # a second write of samples [2, 4) changes exactly those samples at every level
        images[2:4] = rs.randint(0, 256, size=(2, Hs, Ws, 3)).astype(np.uint8)
        ds.write(2, images[2:4])
        for l, lv in enumerate(M.chain(images, L)):
            assert np.array_equal(ds.read_level(l, 0, n), lv), l
            assert np.array_equal(ds.read_level(l, 3, 2), lv[3:5]), l
        # a labels-only write launches nothing and changes no level
        _, counts = RG.logged(capi, T, lambda: ds.write(1, labels=[7, 8, 9]))
        assert counts == {}, counts
        for l, lv in enumerate(M.chain(images, L)):
            assert np.array_equal(ds.read_level(l, 0, n), lv), l
        assert np.array_equal(ds.read(0, n)[1], [0, 7, 8, 9, 4])
        # refusals: levels that do not exist, ranges outside the dataset, more levels than the size has
        for bad in (-1, L):
            with pytest.raises(capi.CnnAmdError, match="level"):
                ds.read_level(bad, 0, 1)
            with pytest.raises(capi.CnnAmdError, match="level"):
                ds.level_shape(bad)
        with pytest.raises(capi.CnnAmdError, match="outside"):
            ds.read_level(0, n, 1)
        for bad in (0, L + 1):
            with pytest.raises(capi.CnnAmdError, match="levels"):
                capi.ResidentDataset(n, Hs, Ws, levels=bad)
    finally:
        ds.close()


# ---- 2. one level, or maps that stay on level 0: the resident stager as it was ----------------------------------------------------------
IDENTITY_MAPS = ["hflip", "half_pixel", "rotate30_scale1.5", "photo"]


def small_scale_set(which, Hs, Ws, H, W, nb):
    """RG.parameter_set with every map's scale below 2"""
    from cnn_amd import capi

    if which == "rotate30_scale1.5":
        mats, blocks, norm = RG.parameter_set("presets", Hs, Ws, H, W, nb)
        mats[:] = capi.augment_matrix([(capi.AUG_ROTATE, 30.0)], Hs, Ws, 6, 6)
    elif which == "photo":
        mats, blocks, norm = RG.parameter_set("photo", Hs, Ws, H, W, nb)
        mats[:] = capi.augment_matrix([(capi.AUG_ROTATE, 10.0)], Hs, Ws, 6, 6)
    else:
        mats, blocks, norm = RG.parameter_set(which, Hs, Ws, H, W, nb)
    assert all(M.choose(m, 3)[0] == 0 for m in mats)
    return mats, blocks, norm


@pytest.mark.parametrize("which", IDENTITY_MAPS)
@pytest.mark.parametrize("H, W", OUTS, ids=["quad_4x8", "px_3x5"])
def test_one_level_identity(T, H, W, which):
    from cnn_amd import capi

    Hs, Ws = 9, 9
    one, images, labels = make_dataset(RG.N, Hs, Ws, 1, 200)
    three, _, _ = make_dataset(RG.N, Hs, Ws, 3, 200)
    mats, blocks, norm = small_scale_set(which, Hs, Ws, H, W, RG.B)
    want, want_lab = RG.reference(images, labels, RG.IDX, mats, blocks, norm, H, W)
    st1, st3 = RG.resident_stager(one, H, W, norm=norm), RG.resident_stager(three, H, W, norm=norm)
    try:
        (got1, lab1), counts1 = RG.logged(capi, T, lambda: RG.gather(T, st1, RG.IDX, H, W, mats, blocks))
        (got3, lab3), counts3 = RG.logged(capi, T, lambda: RG.gather(T, st3, RG.IDX, H, W, mats, blocks))
        assert counts1 == {"augment_u8_resident": 1}, counts1
        assert counts3 == {"augment_u8_resident_levels": 1}, counts3
        assert got1.tobytes() == want.tobytes() and np.array_equal(lab1, want_lab)
        assert got3.tobytes() == want.tobytes() and np.array_equal(lab3, want_lab)
        with pytest.raises(capi.CnnAmdError, match="one level"):
            st1.levels(0)
        assert np.array_equal(st3.levels(0), np.zeros(RG.B, np.int32))
        host, slot = st3.acquire()  # the caller's maps are not overwritten by submit()
        st3.indices(slot)[:] = RG.IDX
        st3.matrices(slot)[:] = mats
        st3.submit(slot)
        assert st3.matrices(slot).tobytes() == mats.tobytes()
        T.cuda.synchronize()
    finally:
        st1.close()
        st3.close()
        one.close()
        three.close()
    for other in (capi.BatchStager(u8_shape=(RG.B, H, W), depth=2, photo=True), capi.BatchStager(u8_shape=(RG.B, H, W), depth=2)):
        other.B = RG.B
        with pytest.raises(capi.CnnAmdError, match="not a resident stager"):
            other.levels(0)
        other.close()


# ---- 3. a batch whose samples sit on different levels ------------------------------------------------------------------------------------
MIX_HS, MIX_WS, MIX_L, MIX_N = 40, 56, 4, 7
MIX_IDX = np.array([6, 0, 3, 3, 1, -1], np.int32)


def mixed_maps(H, W):
    """identity crop, shrink 2, shrink 4, shrink 5.6 turned by 30 degrees about the source's centre, a mirrored shrink 3, shrink 4"""
    from cnn_amd import capi

    c, s = 5.6 * np.cos(np.pi / 6), 5.6 * np.sin(np.pi / 6)
    cx, cy, ox, oy = (MIX_WS - 1) / 2, (MIX_HS - 1) / 2, (W - 1) / 2, (H - 1) / 2
    return np.array([[1, 0, 3, 0, 1, 2],
                     capi.augment_matrix([], MIX_HS, MIX_WS, 20, 28),
                     capi.augment_matrix([], MIX_HS, MIX_WS, 10, 14),
                     [c, -s, cx - (c * ox - s * oy), s, c, cy - (s * ox + c * oy)],
                     [-3, 0, 50, 0, 3, 1],
                     capi.augment_matrix([], MIX_HS, MIX_WS, 10, 14)], F)


@pytest.fixture(scope="module")
def mixed_store():
    ds, images, labels = make_dataset(MIX_N, MIX_HS, MIX_WS, MIX_L, 300)
    yield ds, images, labels
    ds.close()


@pytest.mark.parametrize("H, W", [(10, 12), (9, 11)], ids=["quad_10x12", "px_9x11"])
def test_mixed_levels_in_one_batch(T, mixed_store, H, W):
    from cnn_amd import capi

    ds, images, labels = mixed_store
    nb = len(MIX_IDX)
    mats = mixed_maps(H, W)
    blocks = np.tile(P.IDENTITY, (nb, 1))
    for b in range(nb):
        blocks[b, :12] = capi.colour_matrix([(capi.COL_BRIGHTNESS, 1.3 - 0.1 * b), (capi.COL_CONTRAST, 1.6, 0.5), (capi.COL_SATURATION, 0.5 + 0.2 * b),
                                             (capi.COL_HUE, 15.0 * (b + 1))])
        blocks[b, 12:19] = (2, 1, 3, 2, 10.0 + b, 20.0 + b, 30.0 + b)  # an erase box whose edges cut a quad of four output pixels
    s, t = P.normalize_consts(MEAN, STD)
    want, want_lab, want_lev = M.resident_levels(images, labels, MIX_IDX, mats, blocks, H, W, MIX_L, FILL, s, t, True)
    assert want_lev.tolist() == [0, 1, 2, 2, 1, 2] and want_lab.tolist() == [16, 10, 13, 13, 11, -1]
    st = RG.resident_stager(ds, H, W, nb=nb, norm=(MEAN, STD, True))
    try:
        slot, dev = RG.submit(st, MIX_IDX, mats, blocks)
        levels = st.levels(slot)
        (got, lab), counts = RG.logged(capi, T, lambda: RG.gather(T, st, MIX_IDX, H, W, mats, blocks))
        first, first_lab = RG.collect(T, st, slot, dev, (nb, 3, H, W))
    finally:
        st.close()
    assert counts == {"augment_u8_resident_levels": 1}, counts
    assert np.array_equal(levels, want_lev)
    assert np.array_equal(levels, [capi.augment_level(m, MIX_L)[0] for m in mats])
    assert got.tobytes() == want.tobytes() and np.array_equal(lab, want_lab)
    assert first.tobytes() == want.tobytes() and np.array_equal(first_lab, want_lab)
    # the samples above level 0 are not what level 0 gives through the same maps: the levels are in use
    plain, _ = RG.RR.resident(images, labels, MIX_IDX, mats, blocks, H, W, FILL, s, t, True)
    assert all(got[b].tobytes() != plain[b].tobytes() for b in (1, 2, 3, 4)) and got[0].tobytes() == plain[0].tobytes()


# ---- 4. tiny levels and the bound of the pulled-back load --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_store():
    ds, images, labels = make_dataset(RG.N, 3, 5, 3, 400)
    yield ds, images, labels
    ds.close()


@pytest.mark.parametrize("level", [1, 2], ids=["level1_18_bytes", "level2_6_bytes"])
@pytest.mark.parametrize("H, W", OUTS, ids=["quad_4x8", "px_3x5"])
def test_tiny_levels_and_the_load_bound(T, tiny_store, H, W, level):
    """source 3 x 5, levels 2 x 3 (18 bytes: 8-byte loads, the last one pulled back) and 1 x 2 (6 bytes: byte loads).  RG.IDX reads the
    last sample of the store -- at level 2 its last byte is the allocation's last -- the first, an absent one, and sample 3 twice, whose
    neighbour behind it holds other bytes"""
    ds, images, labels = tiny_store
    Hl, Wl = ds.level_shape(level)
    assert (Hl, Wl, Hl * Wl * 3) == ((2, 3, 18) if level == 1 else (1, 2, 6))
    mats = np.tile(level_shift_map(level, Hl, Wl, H, W), (RG.B, 1))
    blocks = np.tile(P.IDENTITY, (RG.B, 1))
    want, want_lab, want_lev = M.resident_levels(images, labels, RG.IDX, mats, blocks, H, W, 3, FILL)
    assert (want_lev == level).all()
    lv = M.chain(images, 3)[level]
    last = R.plain(lv[RG.IDX[0]][None])[0][:, Hl - 1, Wl - 1]  # the last output pixel is the level's last pixel (both taps, both rows)
    assert want[0, :, H - 1, W - 1].tobytes() == last.tobytes()
    assert not np.array_equal(lv[3], lv[4])
    st = RG.resident_stager(ds, H, W)
    try:
        got, lab = RG.gather(T, st, RG.IDX, H, W, mats, blocks)
    finally:
        st.close()
    assert got.tobytes() == want.tobytes() and np.array_equal(lab, want_lab)


# ---- 5. it antialiases -----------------------------------------------------------------------------------------------------------------
def test_it_antialiases(T):
    """columns 0, 255, 255, 0 repeated, resized 64 -> 16.  One level: sx = 4x + 1.5, the two taps are columns 4x + 1 and 4x + 2, both 255:
    exactly 1.0 everywhere, the dark half of the image is never read.  Three levels: (0 + 255 + 0 + 255 + 2) >> 2 = 128 at level 1,
    (4 * 128 + 2) >> 2 = 128 at level 2, and the map on level 2 is the identity: exactly lut[128] everywhere"""
    from cnn_amd import capi

    col = np.tile(np.array([0, 255, 255, 0], np.uint8), 16)
    image = np.broadcast_to(col[None, None, :, None], (1, 64, 64, 3)).copy()
    lut128 = F(128) * F(1.0) / F(255)
    out = {}
    for L in (1, 3):
        ds = capi.ResidentDataset(1, 64, 64, levels=L)
        ds.write(0, image, [0])
        st = capi.BatchStager(u8_shape=(1, 16, 16), resident=ds, depth=2)
        try:
            out[L], _ = RG.gather(T, st, np.array([0], np.int32), 16, 16)  # the presets: the plain resize map
        finally:
            st.close()
            ds.close()
    assert out[3].tobytes() == np.full((1, 3, 16, 16), lut128, F).tobytes()
    assert out[1].tobytes() == np.full((1, 3, 16, 16), 1.0, F).tobytes()


# ---- 6. beyond 2^32 inside a higher level -----------------------------------------------------------------------------------------------
BIG_N, BIG = 5600, 1024
BIG_SAMPLES = (0, 5461, 5462, 5599)


def test_offsets_beyond_4_gib_inside_level_1(T):
    from cnn_amd import capi
    from tests import large

    half = (BIG // 2) * (BIG // 2) * 3
    assert half == 786432 and 5461 * half < (1 << 32) < 5462 * half  # sample 5461 of level 1 crosses byte 2^32, 5462 lies behind it
    large.require_memory(T, BIG_N * (BIG * BIG * 3 + half), "the resident dataset of 5600 images with a second level")
    rs = np.random.RandomState(600)
    written = rs.randint(0, 256, size=(len(BIG_SAMPLES), BIG, BIG, 3), dtype=np.uint8)
    labels = np.arange(1, 1 + len(BIG_SAMPLES), dtype=np.int32)
    level1 = M.halve(written)
    ds = capi.ResidentDataset(BIG_N, BIG, BIG, levels=2)
    try:
        ds.write(0, written[0:1], labels[0:1])
        ds.write(5461, written[1:3], labels[1:3])
        ds.write(5599, written[3:4], labels[3:4])
        for k, i in enumerate(BIG_SAMPLES):
            assert np.array_equal(ds.read_level(1, i, 1)[0], level1[k]), i
        assert not ds.read_level(1, 5460, 1).any() and not ds.read_level(1, 5463, 1).any()
        H = W = 8
        mats = np.tile(level_shift_map(1, BIG // 2, BIG // 2, H, W), (4, 1))
        blocks = np.tile(P.IDENTITY, (4, 1))
        want, want_lab, want_lev = M.resident_levels(written, labels, np.arange(4), mats, blocks, H, W, 2)
        assert (want_lev == 1).all()
        st = RG.resident_stager(ds, H, W, nb=4, fill=0.0)
        try:
            got, lab = RG.gather(T, st, np.array(BIG_SAMPLES, np.int32), H, W, mats, blocks)
        finally:
            st.close()
    finally:
        ds.close()
        large.release(T)
    assert got.tobytes() == want.tobytes() and np.array_equal(lab, want_lab)
    assert len({got[b].tobytes() for b in range(4)}) == 4


# ---- 7. write waits for submitted gathers, at a higher level ------------------------------------------------------------------------------
def test_write_waits_for_submitted_gathers_at_level_2(T):
    """the existing rule (tests/test_gpu_resident.py::test_write_waits_for_submitted_gathers) where the bytes a batch reads are level 2's:
    the rebuild runs behind the same wait.  512 -> 128 is the identity on level 2, so the batch is the plain conversion of that level"""
    from cnn_amd import capi

    nb, hw = 8, 512
    rs = np.random.RandomState(700)
    old = rs.randint(0, 256, size=(nb, hw, hw, 3), dtype=np.uint8)
    new = rs.randint(0, 256, size=(nb, hw, hw, 3), dtype=np.uint8)
    ds = capi.ResidentDataset(nb, hw, hw, levels=3)
    ds.write(0, old, np.arange(nb))
    st = RG.resident_stager(ds, hw // 4, hw // 4, nb=nb, fill=0.0)
    idx = np.arange(nb, dtype=np.int32)
    try:
        slot, dev = RG.submit(st, idx)
        assert (st.levels(slot) == 2).all()
        ds.write(0, new, np.arange(nb) + 100)  # immediately: the gather above is still to run, or running
        first, first_lab = RG.collect(T, st, slot, dev, (nb, 3, hw // 4, hw // 4))
        second, second_lab = RG.gather(T, st, idx, hw // 4, hw // 4)
    finally:
        st.close()
        ds.close()
    assert first.tobytes() == R.plain(M.chain(old, 3)[2]).tobytes() and np.array_equal(first_lab, np.arange(nb))
    assert second.tobytes() == R.plain(M.chain(new, 3)[2]).tobytes() and np.array_equal(second_lab, np.arange(nb) + 100)
