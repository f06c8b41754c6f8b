"""The photo stager (include/cnn_amd.h: cnn_batch_stager_create_u8_photo / _photo / _set_normalize) on the device, through
cnn_amd.capi: colour map, clamp, normalisation and erase box in the gather kernel's epilogue.  Every comparison is torch.equal: the
rule leaves no freedom (tests/photo_ref.py restates it in NumPy behind tests/augment_ref.py, one rounding per operation), and with
the block acquire() presets it yields the geometric stager's bits.  Each batch goes acquire -> fill -> submit -> wait -> cnn_memcpy_d2d
out -> release.  Shapes, the geometric tests' own: B = 3 sources of 7x9, outputs 8x12 (16-byte stores) and 5x7 (W % 4 != 0: per-pixel
stores), and one case with B = 2, 16x16 -> 224x224 (49 workgroups per sample)."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import augment_ref as R
from tests import photo_ref as P
from tests import stream_order as SO

pytestmark = pytest.mark.gpu

FILL = -1.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # ImageNet's
OUTS = [(8, 12), (5, 7)]
OUT_IDS = ["quad_8x12", "tail_5x7"]


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture(scope="module")
def src():
    return np.random.RandomState(11).randint(0, 256, size=(3, 7, 9, 3)).astype(np.uint8)


def submit(st, src, mats=None, photo=None):
    """acquire / fill / submit -> (slot, device pointer)"""
    host, slot = st.acquire()
    host[:] = src.reshape(-1)
    if mats is not None:
        st.matrices(slot)[:] = mats
    if photo is not None:
        st.photo(slot)[:] = photo
    return slot, st.submit(slot)


def collect(T, st, slot, dev, shape):
    """wait / copy out / release -> the batch"""
    from cnn_amd import capi

    st.wait(slot)
    got = T.empty(shape, device="cuda")
    capi.check(capi.load().cnn_memcpy_d2d(got.data_ptr(), dev, got.numel() * 4, capi._stream()), "cnn_memcpy_d2d")
    st.release(slot)
    T.cuda.synchronize()
    return got


def staged(T, st, src, H, W, mats=None, photo=None):
    slot, dev = submit(st, src, mats, photo)
    return collect(T, st, slot, dev, (src.shape[0], 3, H, W))


def photo_stager(src, H, W, fill=FILL):
    from cnn_amd import capi

    B, Hs, Ws, _ = src.shape
    st = capi.BatchStager(u8_shape=(B, H, W), source_shape=(Hs, Ws), depth=2, photo=True)
    st.set_fill(fill)
    return st


def same(T, got, want_np):
    return T.equal(got.cpu(), T.from_numpy(np.ascontiguousarray(want_np)))


def rotations(Hs, Ws, H, W, B):
    from cnn_amd import capi

    return np.stack([capi.augment_matrix([(capi.AUG_ROTATE, 10.0 + 7.0 * b)], Hs, Ws, H, W) for b in range(B)])


def jitter(B):
    """strong per-sample colour maps: with random bytes some values leave [0, 1] on either side"""
    from cnn_amd import capi

    p = np.tile(P.IDENTITY, (B, 1))
    for b in range(B):
        p[b, :12] = capi.colour_matrix([(capi.COL_BRIGHTNESS, 1.3 - 0.2 * b), (capi.COL_CONTRAST, 1.8 + 0.1 * b, 0.5), (capi.COL_SATURATION, 1.5 - 0.4 * b),
                                        (capi.COL_HUE, 20.0 * (b + 1))])
    return p


@pytest.mark.parametrize("H, W", OUTS, ids=OUT_IDS)
def test_the_preset_block_equals_the_geometric_stager(T, src, H, W):
    """an untouched photo block, default normalisation: the bits of cnn_batch_stager_create_u8_aug under a rotation of 10 .. 24 degrees"""
    from cnn_amd import capi

    mats = rotations(7, 9, H, W, 3)
    want, inside = R.augment(src, mats, H, W, FILL)
    assert 0.0 < 1.0 - float(inside.mean()) < 0.5  # some fill, mostly bilinear taps
    geo = capi.BatchStager(u8_shape=(3, H, W), source_shape=(7, 9), depth=2)
    geo.set_fill(FILL)
    st = photo_stager(src, H, W)
    host, slot = st.acquire()
    assert np.array_equal(st.photo(slot), np.tile(P.IDENTITY, (3, 1)))
    st.release(slot)
    a, b = staged(T, geo, src, H, W, mats), staged(T, st, src, H, W, mats)
    geo.close()
    st.close()
    assert same(T, a, want) and T.equal(a, b)
    # the restatement says the same identity
    assert np.array_equal(P.photo(src, mats, np.tile(P.IDENTITY, (3, 1)), H, W, FILL)[0], want)


def test_the_preset_block_equals_the_geometric_stager_at_the_workload_plane(T):
    """B = 2, 16x16 -> 224x224: 49 workgroups per sample; then the same plane with a colour map, normalisation and a box"""
    from cnn_amd import capi

    big = np.random.RandomState(12).randint(0, 256, size=(2, 16, 16, 3)).astype(np.uint8)
    mats = rotations(16, 16, 224, 224, 2)
    want, inside = R.augment(big, mats, 224, 224, FILL)
    assert 0.0 < 1.0 - float(inside.mean()) < 0.5
    geo = capi.BatchStager(u8_shape=(2, 224, 224), source_shape=(16, 16), depth=2)
    geo.set_fill(FILL)
    st = photo_stager(big, 224, 224)
    a, b = staged(T, geo, big, 224, 224, mats), staged(T, st, big, 224, 224, mats)
    geo.close()
    assert same(T, a, want) and T.equal(a, b)
    p = jitter(2)
    p[0, 12:19] = (50, 200, 101, 60, 3.0, 4.0, 5.0)  # cuts quads on both sides, runs past the bottom
    p[1, 12:19] = (222, 0, 2, 224, -3.0, -4.0, -5.0)  # the last two columns
    s, t = P.normalize_consts(MEAN, STD)
    st.set_normalize(MEAN, STD, clamp=True)
    want, _, box, _ = P.photo(big, mats, p, 224, 224, FILL, s, t, True)
    assert box[0].sum() == 101 * 24 and box[1].sum() == 2 * 224
    got = staged(T, st, big, 224, 224, mats, p)
    st.close()
    assert same(T, got, want)


@pytest.mark.parametrize("route", ["one_tap", "bilinear"])
@pytest.mark.parametrize("H, W", OUTS, ids=OUT_IDS)
def test_colour_map_clamp_and_normalisation_equal_the_restatement(T, src, H, W, route):
    if route == "one_tap":
        mats = np.array([[1, 0, 0, 0, 1, 0], [1, 0, -1, 0, 1, 1], [1, 0, 2, 0, 1, -1]], np.float32)  # whole source pixels
    else:
        mats = rotations(7, 9, H, W, 3)
    p = jitter(3)
    s, t = P.normalize_consts(MEAN, STD)
    want, inside, box, raw = P.photo(src, mats, p, H, W, FILL, s, t, True)
    live = np.broadcast_to(inside[:, None], raw.shape)
    assert not box.any() and inside.any() and not inside.all()
    # asked of the reference alone: the clamp bites on both sides and leaves values in between
    low, high, mid = int((raw[live] < 0).sum()), int((raw[live] > 1).sum()), int(((raw[live] > 0) & (raw[live] < 1)).sum())
    assert low > 0 and high > 0 and mid > 0, (low, high, mid)
    st = photo_stager(src, H, W)
    st.set_normalize(MEAN, STD, clamp=True)
    got = staged(T, st, src, H, W, mats, p)
    st.close()
    assert same(T, got, want)


@pytest.mark.parametrize("H, W", OUTS, ids=OUT_IDS)
def test_fill_is_untouched_by_colour_and_normalisation(T, src, H, W):
    mats = np.array([[1, 0, 3, 0, 1, 0], [1, 0, -2, 0, 1, 1], [1, 0, 0, 0, 1, -3]], np.float32)
    s, t = P.normalize_consts(MEAN, STD)
    want, inside, _, _ = P.photo(src, mats, jitter(3), H, W, 0.25, s, t, True)
    outside = np.broadcast_to(~inside[:, None], want.shape)
    assert all(0 < (~inside[b]).sum() < H * W for b in range(3))
    st = photo_stager(src, H, W, fill=0.25)
    st.set_normalize(MEAN, STD, clamp=True)
    got = staged(T, st, src, H, W, mats, jitter(3))
    st.close()
    assert same(T, got, want)
    assert (got.cpu().numpy()[outside] == np.float32(0.25)).all()


@pytest.mark.parametrize("H, W", OUTS, ids=OUT_IDS)
def test_erase_boxes(T, src, H, W):
    """every sample its own box and its own three values"""
    s, t = P.normalize_consts(MEAN, STD)
    mats = rotations(7, 9, H, W, 3)
    ev = np.array([[10, 20, 30], [11, 21, 31], [12, 22, 32]], np.float32)
    st = photo_stager(src, H, W)
    st.set_normalize(MEAN, STD, clamp=True)
    nobox, _, _, _ = P.photo(src, mats, jitter(3), H, W, FILL, s, t, True)

    # a box that runs past the right and bottom edges; a box that cuts a store quad; a box over the whole output
    p = jitter(3)
    cut = (2, 1, 5, 3) if W == 12 else (2, 1, 3, 2)
    p[0, 12:16] = (W - 3, H - 3, 10, 10)
    p[1, 12:16] = cut
    p[2, 12:16] = (0, 0, W, H)
    p[:, 16:19] = ev
    want, _, box, _ = P.photo(src, mats, p, H, W, FILL, s, t, True)
    assert box[0].sum() == 9 and box[1].sum() == cut[2] * cut[3] and box[2].all()
    assert np.array_equal(want[1, :, 0], nobox[1, :, 0])  # the rows of the next sample behind the clipped box are what they were
    for b in range(3):
        for c in range(3):
            assert (want[b, c][box[b]] == ev[b, c]).all() and np.array_equal(want[b, c][~box[b]], nobox[b, c][~box[b]])
    got = staged(T, st, src, H, W, mats, p)
    assert same(T, got, want)

    # ew == 0 and eh == 0 with everything else set: no box; a box over fill pixels: the box wins
    p = jitter(3)
    p[0, 12:16] = (1, 1, 0, 3)
    p[1, 12:16] = (0, 0, 3, H)
    p[2, 12:16] = (1, 1, 3, 0)
    p[:, 16:19] = ev
    shift = mats.copy()
    shift[1] = (1, 0, -2, 0, 1, 0)  # the first two columns leave the source
    want, inside, box, _ = P.photo(src, shift, p, H, W, FILL, s, t, True)
    assert not box[0].any() and not box[2].any() and box[1].sum() == 3 * H
    assert (~inside[1][:, :2]).all() and inside[1][:, 2].any() and (want[1, :, :, :3] == ev[1][:, None, None]).all()
    got = staged(T, st, src, H, W, shift, p)
    st.close()
    assert same(T, got, want)


def test_set_normalize_applies_to_later_submits_only(T, src):
    """two slots in flight, the constants changed between their submits"""
    H, W = 8, 12
    mats, p = rotations(7, 9, H, W, 3), jitter(3)
    st = photo_stager(src, H, W)
    slot0, dev0 = submit(st, src, mats, p)
    st.set_normalize(MEAN, STD, clamp=True)
    slot1, dev1 = submit(st, src, mats, p)
    assert slot0 != slot1
    first, second = collect(T, st, slot0, dev0, (3, 3, H, W)), collect(T, st, slot1, dev1, (3, 3, H, W))
    st.close()
    s, t = P.normalize_consts(MEAN, STD)
    want0, want1 = P.photo(src, mats, p, H, W, FILL)[0], P.photo(src, mats, p, H, W, FILL, s, t, True)[0]
    assert not np.array_equal(want0, want1)
    assert same(T, first, want0) and same(T, second, want1)


@pytest.mark.parametrize("H, W", OUTS, ids=OUT_IDS)
def test_without_the_clamp_values_outside_the_unit_range_survive(T, src, H, W):
    mats, p = rotations(7, 9, H, W, 3), jitter(3)
    want, inside, _, raw = P.photo(src, mats, p, H, W, FILL)
    assert np.array_equal(want, np.where(inside[:, None], raw, np.float32(FILL)))  # s = 1, t = 0: u itself
    live = raw[np.broadcast_to(inside[:, None], raw.shape)]
    assert (live > 1).any() and (live < 0).any()
    st = photo_stager(src, H, W)
    got = staged(T, st, src, H, W, mats, p)
    assert same(T, got, want)
    # and with a normalisation but no clamp
    s, t = P.normalize_consts(MEAN, STD)
    st.set_normalize(MEAN, STD, clamp=False)
    got = staged(T, st, src, H, W, mats, p)
    st.close()
    assert same(T, got, P.photo(src, mats, p, H, W, FILL, s, t, False)[0])


def test_refusals(T):
    from cnn_amd import capi

    for st in (capi.BatchStager(u8_shape=(3, 7, 9), depth=2), capi.BatchStager(u8_shape=(3, 7, 9), depth=2, augment=True),
               capi.BatchStager(3 * 3 * 7 * 9 * 4, depth=2)):
        st.B = 3
        with pytest.raises(capi.CnnAmdError, match="not a photo stager"):
            st.photo(0)
        with pytest.raises(capi.CnnAmdError, match="not a photo stager"):
            st.set_normalize(MEAN, STD)
        st.close()
    st = capi.BatchStager(u8_shape=(3, 7, 9), depth=2, photo=True)
    assert st.matrices(0).shape == (3, 6) and st.photo(1).shape == (3, 20)
    for mean, std in ((MEAN, (0.2, 0.0, 0.2)), (MEAN, (0.2, float("nan"), 0.2)), ((0.0, float("inf"), 0.0), STD), (MEAN, (1e-45, 1.0, 1.0))):
        with pytest.raises(capi.CnnAmdError, match="finite"):
            st.set_normalize(mean, std)
    with pytest.raises(capi.CnnAmdError, match="bad arguments"):
        st.photo(2)
    lib = capi.load()
    assert lib.cnn_batch_stager_set_normalize(st.h, None, None, 1) == 1 and b"null" in lib.cnn_amd_last_error()
    st.close()


@pytest.fixture
def H_(T):
    h = SO.harness(T)
    try:
        yield h
    finally:
        h.finish()


def test_photo_stager_wait_orders_the_consumer_behind_the_submit(T, H_):
    """tests/test_gpu_stream_order_plumbing.py::test_stager_wait_orders_the_consumer_behind_the_upload for the photo kind: wait(slot, S)
    in front of a consumer on S.  The stager's stream is out of a gate's reach, so the submit itself is long (25 MB of bytes, the kernel
    and 100 MB of floats, about a millisecond) against a consumer queued tens of microseconds behind it.  The consumer -- a copy of
    the slot on S -- holds the new batch, brightened by the slot's own block; one that did not wait would copy a slot in the middle of
    its upload.  Liveness as there: the host-side time from submit() to the queued consumer is at most a quarter of the submit's own
    time, and the consumer is still pending when the host returns"""
    from cnn_amd import capi

    lib = capi.load()
    stager = capi.BatchStager(depth=2, u8_shape=(8, 1024, 1024), photo=True)
    rs = np.random.RandomState(8500)
    old_in = rs.randint(0, 256, size=(8, 1024, 1024, 3), dtype=np.uint8)
    new_in = rs.randint(0, 256, size=(8, 1024, 1024, 3), dtype=np.uint8)
    block = np.tile(P.IDENTITY, (8, 1))
    block[:, [0, 4, 8]] = 0.5  # exact in fp32: out = 0.5 * lut[byte]
    new_out = (np.float32(0.5) * R.plain(new_in)).reshape(-1)
    n = new_out.size
    try:
        with T.cuda.stream(H_.S):
            host, slot = stager.acquire()
            host[:] = old_in.reshape(-1)
            T.cuda.synchronize()
            t0 = time.perf_counter()
            dev_ptr = stager.submit(slot)
            stager.wait(slot)
            H_.S.synchronize()
            upload_ms = (time.perf_counter() - t0) * 1e3
            stager.release(slot)
            host, slot = stager.acquire()  # (the other slot: free)
            host[:] = new_in.reshape(-1)
            stager.photo(slot)[:] = block
            seen = T.full((n,), 7.0, device="cuda")
            T.cuda.synchronize()
            t0 = time.perf_counter()
            dev_ptr = stager.submit(slot)
            stager.wait(slot)
            capi.check(lib.cnn_memcpy_d2d(capi._ptr(seen), C.c_void_p(dev_ptr), n * 4, capi._stream()), "cnn_memcpy_d2d")
            done = T.cuda.Event()
            done.record(H_.S)
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            pending = not done.query()
            stager.release(slot)
        H_.S.synchronize()
        H_.enqueue_ms["stager wait u8_photo"] = (enqueue_ms, upload_ms)
        assert pending and 4 * enqueue_ms <= upload_ms, f"the submit ({upload_ms:.3f} ms) was over before the consumer was queued ({enqueue_ms:.3f} ms): nothing proven"
        assert seen.cpu().numpy().tobytes() == new_out.astype(np.float32).tobytes(), "the consumer behind wait() did not see its batch"
    finally:
        T.cuda.synchronize()
        stager.close()
