"""The device-resident dataset and its stager (include/cnn_amd.h: cnn_dataset_* and cnn_batch_stager_create_u8_resident / _indices /
_labels) on the device, through cnn_amd.capi and cnn_amd.hostapi.  Every comparison is bit for bit: tests/resident_ref.py restates the
rule (tests/photo_ref.py behind tests/augment_ref.py applied to images[idx]).  Each batch goes acquire -> indices / parameters -> submit
-> wait -> cnn_memcpy_d2d out -> release.  The shapes are the smallest at which each route of the kernel runs: a dataset of N = 7
samples of 1x2 (under 8 bytes per sample: byte loads), 5x7 and 9x9, outputs of 4x8 (16-byte stores) and 3x5 (per-pixel stores), B = 5
with the indices [6, 0, -1, 3, 3]: the last sample of the store, the first, an absent one, and one twice with a neighbour behind it."""
import numpy as np
import pytest

from tests import augment_ref as R
from tests import photo_ref as P
from tests import resident_ref as RR

pytestmark = pytest.mark.gpu

N = 7
IDX = np.array([6, 0, -1, 3, 3], np.int32)
B = 5
FILL = -1.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # ImageNet's
SOURCES = [(1, 2), (5, 7), (9, 9)]
OUTS = [(4, 8), (3, 5)]
PARAMS = ["presets", "hflip", "half_pixel", "rotate30", "photo"]
GIB = 1 << 30


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def make_dataset(Hs, Ws, seed, n=N):
    """-> (capi.ResidentDataset, images, labels): random bytes, every sample its own, labels 10 .. 10 + n - 1"""
    from cnn_amd import capi

    images = np.random.RandomState(seed).randint(0, 256, size=(n, Hs, Ws, 3)).astype(np.uint8)
    assert all(not np.array_equal(images[i], images[i + 1]) for i in range(n - 1))
    labels = np.arange(10, 10 + n, dtype=np.int32)
    ds = capi.ResidentDataset(n, Hs, Ws)
    ds.write(0, images, labels)
    return ds, images, labels


def submit(st, idx, mats=None, photo=None):
    host, slot = st.acquire()
    assert host is None
    st.indices(slot)[:] = idx
    if mats is not None:
        st.matrices(slot)[:] = mats
    if photo is not None:
        st.photo(slot)[:] = photo
    return slot, st.submit(slot)


def collect(T, st, slot, dev, shape):
    """wait / copy the batch and its labels out / release -> (batch, labels) as NumPy"""
    import ctypes as C

    from cnn_amd import capi

    st.wait(slot)
    got = T.empty(shape, device="cuda")
    lab = T.empty((shape[0],), dtype=T.int32, device="cuda")
    lib = capi.load()
    capi.check(lib.cnn_memcpy_d2d(got.data_ptr(), dev, got.numel() * 4, capi._stream()), "cnn_memcpy_d2d")
    capi.check(lib.cnn_memcpy_d2d(lab.data_ptr(), C.c_void_p(st.labels(slot)), lab.numel() * 4, capi._stream()), "cnn_memcpy_d2d")
    st.release(slot)
    T.cuda.synchronize()
    return got.cpu().numpy(), lab.cpu().numpy()


def gather(T, st, idx, H, W, mats=None, photo=None):
    slot, dev = submit(st, idx, mats, photo)
    return collect(T, st, slot, dev, (len(idx), 3, H, W))


def parameter_set(which, Hs, Ws, H, W, nb=B):
    """-> (matrices (nb, 6), photo blocks (nb, 20), normalisation (mean, std, clamp) or None)"""
    from cnn_amd import capi

    blocks = np.tile(P.IDENTITY, (nb, 1))
    norm = None
    if which == "presets":  # what acquire() leaves in the slot: the plain resize map
        m = capi.augment_matrix([], Hs, Ws, H, W)
    elif which == "hflip":  # whole source pixels (no resize): the one-tap route; what lies right of / below the source is fill
        m = np.array([-1, 0, Ws - 1, 0, 1, 0], np.float32)
    elif which == "half_pixel":  # four taps; the LAST output pixel samples (Ws - 0.5, Hs - 0.5): its load ends with the sample
        m = np.array([1, 0, (Ws - 0.5) - (W - 1), 0, 1, (Hs - 0.5) - (H - 1)], np.float32)
    elif which == "rotate30":
        m = capi.augment_matrix([(capi.AUG_ROTATE, 30.0)], Hs, Ws, H, W)
    else:  # a colour map, ImageNet's mean / std, the clamp, and an erase box whose edges cut a quad of four output pixels
        m = capi.augment_matrix([(capi.AUG_ROTATE, 10.0)], Hs, Ws, H, W)
        for b in range(nb):
            blocks[b, :12] = capi.colour_matrix([(capi.COL_BRIGHTNESS, 1.3 - 0.1 * b), (capi.COL_CONTRAST, 1.6, 0.5), (capi.COL_SATURATION, 0.5 + 0.2 * b),
                                                 (capi.COL_HUE, 15.0 * (b + 1))])
            blocks[b, 12:19] = (2, 1, 3, 2, 10.0 + b, 20.0 + b, 30.0 + b)
        norm = (MEAN, STD, True)
    return np.tile(np.asarray(m, np.float32), (nb, 1)), blocks, norm


def reference(images, labels, idx, mats, blocks, norm, H, W, fill=FILL):
    if norm is None:
        return RR.resident(images, labels, idx, mats, blocks, H, W, fill)
    s, t = P.normalize_consts(norm[0], norm[1])
    return RR.resident(images, labels, idx, mats, blocks, H, W, fill, s, t, norm[2])


def resident_stager(ds, H, W, nb=B, norm=None, fill=FILL, depth=2):
    from cnn_amd import capi

    st = capi.BatchStager(u8_shape=(nb, H, W), resident=ds, depth=depth)
    st.set_fill(fill)
    if norm is not None:
        st.set_normalize(*norm)
    return st


def logged(capi, T, fn):
    """fn() with the library's launch log on -> (fn's result, {kernel name: launches})"""
    capi.kernel_timing(1)
    try:
        out = fn()
        T.cuda.synchronize()
        counts = {}
        for key, (n, _ms) in capi.kernel_timing_report().items():
            counts[key.split("|")[0]] = counts.get(key.split("|")[0], 0) + n
    finally:
        capi.kernel_timing(0)
    return out, counts


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SOURCES, ids=[f"src_{h}x{w}" for h, w in SOURCES])
def stored(request):
    Hs, Ws = request.param
    ds, images, labels = make_dataset(Hs, Ws, 100 + Hs)
    yield ds, images, labels
    ds.close()


@pytest.mark.parametrize("which", PARAMS)
@pytest.mark.parametrize("H, W", OUTS, ids=["quad_4x8", "px_3x5"])
def test_bits(T, stored, H, W, which):
    from cnn_amd import capi

    ds, images, labels = stored
    _, Hs, Ws, _ = images.shape
    mats, blocks, norm = parameter_set(which, Hs, Ws, H, W)
    want, want_lab = reference(images, labels, IDX, mats, blocks, norm, H, W)
    assert np.array_equal(want_lab, [16, 10, -1, 13, 13])
    absent = np.where((np.arange(W)[None, :] >= blocks[2, 12]) & (np.arange(W)[None, :] < blocks[2, 12] + blocks[2, 14]) &
                      (np.arange(H)[:, None] >= blocks[2, 13]) & (np.arange(H)[:, None] < blocks[2, 13] + blocks[2, 15]), np.nan, FILL)
    for c in range(3):  # the absent row: fill, and the box's value inside the box
        assert np.array_equal(want[2, c][~np.isnan(absent)], np.full(int((~np.isnan(absent)).sum()), FILL, np.float32))
        assert (want[2, c][np.isnan(absent)] == blocks[2, 16 + c]).all()
    st = resident_stager(ds, H, W, norm=norm)
    try:
        preset = which == "presets"
        (got, lab), counts = logged(capi, T, lambda: gather(T, st, IDX, H, W, None if preset else mats, None if preset else blocks))
    finally:
        st.close()
    assert counts == {"augment_u8_resident": 1}, counts
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(lab, want_lab)


def test_acquire_presets_the_slot(T, stored):
    from cnn_amd import capi

    ds, images, _ = stored
    _, Hs, Ws, _ = images.shape
    st = resident_stager(ds, 4, 8)
    try:
        host, slot = st.acquire()
        assert host is None
        assert np.array_equal(st.indices(slot), np.full(B, -1, np.int32))
        assert np.array_equal(st.matrices(slot), np.tile(capi.augment_matrix([], Hs, Ws, 4, 8), (B, 1)))
        assert np.array_equal(st.photo(slot), np.tile(P.IDENTITY, (B, 1)))
        dev = st.submit(slot)  # every sample absent: a batch of fill, labels of -1, nothing read
        got, lab = collect(T, st, slot, dev, (B, 3, 4, 8))
    finally:
        st.close()
    assert (got == np.float32(FILL)).all() and (lab == -1).all()


# ---- 2. the same bits as the host-fed stager ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", PARAMS)
@pytest.mark.parametrize("H, W", OUTS, ids=["quad_4x8", "px_3x5"])
def test_same_bits_as_the_host_fed_photo_stager(T, stored, H, W, which):
    """the same five images through BatchStager(photo=True) with the same parameters: the four real rows are identical word for word
    (the absent row has no host-fed equivalent -- a zero image's pixels are inside -- and is left out)"""
    import ctypes as C

    from cnn_amd import capi

    ds, images, labels = stored
    _, Hs, Ws, _ = images.shape
    mats, blocks, norm = parameter_set(which, Hs, Ws, H, W)
    st = resident_stager(ds, H, W, norm=norm)
    fed = capi.BatchStager(u8_shape=(B, H, W), source_shape=(Hs, Ws), depth=2, photo=True)
    try:
        fed.set_fill(FILL)
        if norm is not None:
            fed.set_normalize(*norm)
        got, _ = gather(T, st, IDX, H, W, mats, blocks)
        host, slot = fed.acquire()
        host[:] = images[np.where(IDX >= 0, IDX, 0)].reshape(-1)
        fed.matrices(slot)[:] = mats
        fed.photo(slot)[:] = blocks
        dev = fed.submit(slot)
        fed.wait(slot)
        other = T.empty((B, 3, H, W), device="cuda")
        capi.check(capi.load().cnn_memcpy_d2d(other.data_ptr(), C.c_void_p(dev), other.numel() * 4, capi._stream()), "cnn_memcpy_d2d")
        fed.release(slot)
        T.cuda.synchronize()
    finally:
        st.close()
        fed.close()
    real = np.flatnonzero(IDX >= 0)
    assert len(real) == 4
    assert got[real].tobytes() == other.cpu().numpy()[real].tobytes()


# ---- 3. slot reuse ---------------------------------------------------------------------------------------------------------------------
def test_slot_reuse(T):
    """depth 2, six batches in a row, each with its own indices and parameters, read after wait and then released"""
    from cnn_amd import capi

    ds, images, labels = make_dataset(5, 7, 31)
    H, W = 4, 8
    st = resident_stager(ds, H, W)
    rs = np.random.RandomState(32)
    try:
        def run():
            out = []
            for i in range(6):
                idx = rs.randint(-1, N, size=B).astype(np.int32)
                mats, blocks, _ = parameter_set(PARAMS[i % 4], 5, 7, H, W)
                mats[:, 2] += np.float32(0.25 * i)
                blocks[:, 9:12] = np.float32(0.125 * i)
                out.append((idx, mats, blocks, gather(T, st, idx, H, W, mats, blocks)))
            return out

        batches, counts = logged(capi, T, run)
    finally:
        st.close()
        ds.close()
    assert counts == {"augment_u8_resident": 6}, counts
    for i, (idx, mats, blocks, (got, lab)) in enumerate(batches):
        want, want_lab = reference(images, labels, idx, mats, blocks, None, H, W)
        assert got.tobytes() == want.tobytes() and np.array_equal(lab, want_lab), i


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(T):
    import ctypes as C

    from cnn_amd import capi

    lib = capi.load()
    ds, images, labels = make_dataset(5, 7, 41)
    H, W = 4, 8
    st = resident_stager(ds, H, W)
    mats, blocks, _ = parameter_set("presets", 5, 7, H, W)
    try:
        for bad in (N, -2):
            host, slot = st.acquire()
            idx = IDX.copy()
            idx[3] = bad
            st.indices(slot)[:] = idx

            def refused():
                with pytest.raises(capi.CnnAmdError, match="outside"):
                    st.submit(slot)

            _, counts = logged(capi, T, refused)
            assert counts == {}, counts  # nothing was enqueued
            st.indices(slot)[:] = IDX  # the slot is still acquired and usable
            got, lab = collect(T, st, slot, st.submit(slot), (B, 3, H, W))
            want, want_lab = reference(images, labels, IDX, mats, blocks, None, H, W)
            assert got.tobytes() == want.tobytes() and np.array_equal(lab, want_lab)
        # a dataset with a stager attached is not destroyed, and stays usable
        assert lib.cnn_dataset_destroy(ds.h) == 1 and b"attached" in lib.cnn_amd_last_error()
        with pytest.raises(capi.CnnAmdError, match="attached"):
            ds.close()
        assert ds.h and ds.info() == (N, 5, 7)
        got, _ = gather(T, st, IDX, H, W)
        assert got.tobytes() == want.tobytes()
    finally:
        st.close()
    # the other three kinds have no indices and no labels
    for other in (capi.BatchStager(u8_shape=(B, H, W), depth=2, photo=True), capi.BatchStager(u8_shape=(B, H, W), depth=2, augment=True),
                  capi.BatchStager(u8_shape=(B, H, W), depth=2), capi.BatchStager(B * 3 * H * W * 4, depth=2)):
        other.B = B
        with pytest.raises(capi.CnnAmdError, match="not a resident stager"):
            other.indices(0)
        with pytest.raises(capi.CnnAmdError, match="not a resident stager"):
            other.labels(0)
        other.close()
    # ranges
    one = np.zeros((1, 5, 7, 3), np.uint8)
    for first, img in ((N, one), (-1, one), (N - 1, np.zeros((2, 5, 7, 3), np.uint8))):
        with pytest.raises(capi.CnnAmdError, match="outside"):
            ds.write(first, img)
    for first, count in ((0, 0), (0, N + 1), (N, 1), (-1, 1)):
        with pytest.raises(capi.CnnAmdError, match="outside"):
            ds.read(first, count)
    assert lib.cnn_dataset_write(ds.h, 0, 1, None, None) == 1 and b"both null" in lib.cnn_amd_last_error()
    assert lib.cnn_dataset_read(ds.h, 0, 1, None, None) == 1 and b"both null" in lib.cnn_amd_last_error()
    for n, hs, ws in ((0, 5, 7), (1 << 31, 1, 1), (1, 0, 7), (1, 5, 8193)):
        h = C.c_void_p()
        assert lib.cnn_dataset_create_u8(C.byref(h), n, hs, ws) == 1 and not h.value
    # read returns what write wrote; what nothing wrote is 0 / -1
    fresh = capi.ResidentDataset(4, 3, 2)
    part = np.random.RandomState(42).randint(1, 256, size=(2, 3, 2, 3)).astype(np.uint8)
    fresh.write(1, part, [7, 8])
    fresh.write(3, labels=[9])
    img, lab = fresh.read(0, 4)
    assert np.array_equal(img[1:3], part) and not img[0].any() and not img[3].any()
    assert np.array_equal(lab, [-1, 7, 8, 9])
    fresh.write(1, part[::-1])  # images alone: the labels stay
    img, lab = fresh.read(1, 2)
    assert np.array_equal(img, part[::-1]) and np.array_equal(lab, [7, 8])
    fresh.close()
    ds.close()  # no stager attached any more
    assert ds.h is None


# ---- 5. beyond 4 GiB -------------------------------------------------------------------------------------------------------------------
BIG_N, BIG = 1400, 1024  # 1400 samples of 3 MiB: 4.1 GiB; samples 1365 and 1366 straddle byte 2^32


@pytest.fixture(scope="module")
def big_store(T):
    from cnn_amd import capi
    from tests import large

    assert 1365 * BIG * BIG * 3 < (1 << 32) < 1367 * BIG * BIG * 3
    large.require_memory(T, BIG_N * BIG * BIG * 3, "the 4.1 GiB resident dataset")
    ds = capi.ResidentDataset(BIG_N, BIG, BIG)
    yield ds
    ds.close()


def test_offsets_beyond_4_gib(T, big_store):
    ds = big_store
    rs = np.random.RandomState(51)
    written = {i: rs.randint(0, 256, size=(1, BIG, BIG, 3), dtype=np.uint8) for i in (1365, 1366, 1399)}
    ds.write(1365, np.concatenate([written[1365], written[1366]]), [1, 2])
    ds.write(1399, written[1399], [3])
    idx = np.array([1399, 1365, 1366, 0], np.int32)
    from cnn_amd import capi

    mats = np.tile(capi.augment_matrix([], BIG, BIG, 8, 8), (1, 1))
    st = resident_stager(ds, 8, 8, nb=4, fill=0.0)
    try:
        got, lab = gather(T, st, idx, 8, 8)
    finally:
        st.close()
    for b, i in enumerate((1399, 1365, 1366)):
        want = R.augment(written[i], mats, 8, 8, 0.0)[0]
        assert got[b:b + 1].tobytes() == want.tobytes(), i
    zero = R.augment(np.zeros((1, BIG, BIG, 3), np.uint8), mats, 8, 8, 0.0)[0]  # a sample nothing was written to: bytes of 0
    assert got[3:4].tobytes() == zero.tobytes() and not zero.any()
    assert np.array_equal(lab, [3, 1, 2, -1])


# ---- 6. write waits for submitted gathers -------------------------------------------------------------------------------------------------
def test_write_waits_for_submitted_gathers(T):
    from cnn_amd import capi

    nb = 8
    rs = np.random.RandomState(61)
    old = rs.randint(0, 256, size=(nb, BIG, BIG, 3), dtype=np.uint8)
    new = rs.randint(0, 256, size=(nb, BIG, BIG, 3), dtype=np.uint8)
    ds = capi.ResidentDataset(nb, BIG, BIG)
    ds.write(0, old, np.arange(nb))
    st = resident_stager(ds, BIG, BIG, nb=nb, fill=0.0)
    idx = np.arange(nb, dtype=np.int32)
    try:
        slot, dev = submit(st, idx)
        ds.write(0, new, np.arange(nb) + 100)  # immediately: the gather above is still to run, or running
        first, first_lab = collect(T, st, slot, dev, (nb, 3, BIG, BIG))
        second, second_lab = gather(T, st, idx, BIG, BIG)
    finally:
        st.close()
        ds.close()
    assert first.tobytes() == R.plain(old).tobytes() and np.array_equal(first_lab, np.arange(nb))
    assert second.tobytes() == R.plain(new).tobytes() and np.array_equal(second_lab, np.arange(nb) + 100)


# ---- 7. training is the same training ----------------------------------------------------------------------------------------------------
TRAIN_N, TRAIN_B, TRAIN_HW = 16, 4, 64


def _train_net():
    from cnn_amd import hostapi
    from cnn_amd import stacks as S

    spec = S.alexnet(3)
    net = hostapi.HostSequential(spec, (3, TRAIN_HW, TRAIN_HW))
    net.set_params(S.he_init(S.walk(spec, 3, TRAIN_HW, TRAIN_HW), 71))
    return net


def _train_host_fed(T, images, labels, order):
    from cnn_amd import capi

    net = _train_net()
    st = capi.BatchStager(u8_shape=(TRAIN_B, TRAIN_HW, TRAIN_HW), depth=2, photo=True)
    try:
        for row in order:
            host, slot = st.acquire()
            host[:] = images[row].reshape(-1)
            dev = st.submit(slot)
            st.wait(slot)
            lab = T.from_numpy(labels[row]).cuda()
            net.train_step_ptr(dev, lab, TRAIN_B, TRAIN_HW, TRAIN_HW, 1e-2)
            st.release(slot)
        T.cuda.synchronize()
        return net.get_params()
    finally:
        st.close()
        net.close()


def test_training_is_the_same_training(T):
    from cnn_amd import capi, hostapi

    images = np.random.RandomState(72).randint(0, 256, size=(TRAIN_N, TRAIN_HW, TRAIN_HW, 3)).astype(np.uint8)
    labels = (np.arange(TRAIN_N) % 3).astype(np.int32)
    order = hostapi.epoch_order(TRAIN_N, TRAIN_B, 0, 0, shuffle=False, drop_last=True)[:3]
    assert order.shape == (3, TRAIN_B) and np.array_equal(order.reshape(-1), np.arange(12))
    a = _train_host_fed(T, images, labels, order)
    b = _train_host_fed(T, images, labels, order)
    assert a.tobytes() == b.tobytes(), "the premise: two host-fed runs are bit-identical"
    ds = capi.ResidentDataset(TRAIN_N, TRAIN_HW, TRAIN_HW)
    ds.write(0, images, labels)
    st = capi.BatchStager(u8_shape=(TRAIN_B, TRAIN_HW, TRAIN_HW), resident=ds, depth=2)
    net = _train_net()
    try:
        p0 = net.get_params()
        net.train_epoch_resident(st, order, 1e-2)
        T.cuda.synchronize()
        c = net.get_params()
        assert c.tobytes() != p0.tobytes()
        assert c.tobytes() == a.tobytes()
        # a padded order is refused before anything is enqueued
        padded = hostapi.epoch_order(TRAIN_N - 2, TRAIN_B, 0, 0)
        assert (padded == -1).sum() == 2

        def refused():
            with pytest.raises(capi.CnnAmdError, match="-1"):
                net.train_epoch_resident(st, padded, 1e-2)

        _, counts = logged(capi, T, refused)
        assert counts == {}, counts
        assert net.get_params().tobytes() == c.tobytes()
    finally:
        T.cuda.synchronize()
        net.close()
        st.close()
        ds.close()


# ---- 8. evaluation ----------------------------------------------------------------------------------------------------------------------
def test_evaluation(T):
    """N = 10, B = 4: the last row carries two -1; evaluate_resident equals HostNet.evaluate over the same batches built by hand"""
    from cnn_amd import capi, hostapi

    n = 10
    images = np.random.RandomState(81).randint(0, 256, size=(n, TRAIN_HW, TRAIN_HW, 3)).astype(np.uint8)
    labels = (np.arange(n) * 2 % 3).astype(np.int32)
    order = hostapi.epoch_order(n, TRAIN_B, 3, 0)
    assert order.shape == (3, TRAIN_B) and (order[2, 2:] == -1).all() and (order.reshape(-1)[:10] >= 0).all()
    ds = capi.ResidentDataset(n, TRAIN_HW, TRAIN_HW)
    ds.write(0, images, labels)
    st = capi.BatchStager(u8_shape=(TRAIN_B, TRAIN_HW, TRAIN_HW), resident=ds, depth=2)
    net = _train_net()
    try:
        got = net.evaluate_resident(st, order)
        ident = RR.identity_params(TRAIN_B, TRAIN_HW, TRAIN_HW, TRAIN_HW, TRAIN_HW)
        batches = []
        for row in order:
            x, lab = RR.resident(images, labels, row, ident[0], ident[1], TRAIN_HW, TRAIN_HW)
            batches.append((T.from_numpy(x).cuda(), T.from_numpy(lab).cuda()))
        want = net.evaluate(batches)
    finally:
        T.cuda.synchronize()
        net.close()
        st.close()
        ds.close()
    assert want["samples"] == 10 and want["ignored"] == 2
    for key in ("samples", "ignored", "top1", "topk"):
        assert got[key] == want[key], key
    assert np.float64(got["loss_sum"]).tobytes() == np.float64(want["loss_sum"]).tobytes()
    assert np.array_equal(got["confusion"], want["confusion"])
