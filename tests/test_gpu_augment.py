"""cnn_augment_u8 and the augmenting u8 stager (include/cnn_amd.h) on the device, through cnn_amd.capi.  Every comparison is torch.equal:
the rule leaves no freedom (tests/augment_ref.py restates it in NumPy, one rounding per operation), and with integer maps it yields the
plain conversion of the permuted image, which is held to the plain u8 stager's own output.  Sources and matrices sit between poisoned
guard zones and every output is written into one (tests/guarded.py): nothing outside dst may change.  Shapes: 7x9 / 6x6 images (odd
sizes, partial workgroups), 8x12 (16-byte stores) and 5x7 (W % 4 != 0: per-pixel stores) outputs, and one case at the workload's
224x224 plane (49 workgroups per sample)."""
import numpy as np
import pytest

from tests import augment_ref as R
from tests import guarded

pytestmark = pytest.mark.gpu

FILL = -1.0  # no table entry: lut[v] is in [0, 1]


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def images(B, Hs, Ws, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(B, Hs, Ws, 3)).astype(np.uint8)


def run(T, src, mats, H, W, fill=0.0, shift_bytes=0):
    """capi.augment_u8 on guarded operands into a guarded output -> the output tensor (the canaries are checked)"""
    from cnn_amd import capi

    keep = []
    s = guarded.operand(src, guarded.BYTES, keep, "src")
    m = guarded.operand(np.asarray(mats, np.float32), guarded.NAN, keep, "matrices")
    out = guarded.output((src.shape[0], 3, H, W), guarded.NAN, keep, "dst", shift_bytes=shift_bytes)
    got = capi.augment_u8(s, m, H, W, fill, out=out)
    T.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert guarded.check(keep) == []
    return out


def plain_stager_output(T, src):
    """what a plain cnn_batch_stager_create_u8 stager makes of the bytes"""
    from cnn_amd import capi

    B, H, W, _ = src.shape
    st = capi.BatchStager(u8_shape=(B, H, W), depth=2)
    host, slot = st.acquire()
    host[:] = src.reshape(-1)
    dev = st.submit(slot)
    st.wait(slot)
    got = T.empty((B, 3, H, W), device="cuda")
    capi.check(capi.load().cnn_memcpy_d2d(got.data_ptr(), dev, got.numel() * 4, capi._stream()), "cnn_memcpy_d2d")
    st.release(slot)
    T.cuda.synchronize()
    st.close()
    return got


@pytest.fixture(scope="module")
def small(T):
    """B = 3 images of 7x9 and their plain conversion, from the plain stager (held to the NumPy table here, once)"""
    src = images(3, 7, 9, 11)
    plain = plain_stager_output(T, src)
    assert np.array_equal(plain.cpu().numpy(), R.plain(src))
    return src, plain.cpu().numpy()


def same(T, got, want_np):
    return T.equal(got.cpu(), T.from_numpy(np.ascontiguousarray(want_np)))


def test_identity_equals_the_plain_stager(T, small):
    src, plain = small
    assert same(T, run(T, src, [[1, 0, 0, 0, 1, 0]] * 3, 7, 9, FILL), plain)


def test_hflip_per_sample(T, small):
    from cnn_amd import capi

    src, plain = small
    flip, ident = capi.augment_matrix([(capi.AUG_HFLIP,)], 7, 9, 7, 9), capi.augment_matrix([], 7, 9, 7, 9)
    want = plain.copy()
    want[0], want[2] = plain[0][:, :, ::-1], plain[2][:, :, ::-1]
    assert same(T, run(T, src, [flip, ident, flip], 7, 9, FILL), want)


def test_vflip_per_sample(T, small):
    from cnn_amd import capi

    src, plain = small
    v = capi.augment_matrix([(capi.AUG_VFLIP,)], 7, 9, 7, 9)
    hv = capi.augment_matrix([(capi.AUG_VFLIP,), (capi.AUG_HFLIP,)], 7, 9, 7, 9)
    want = plain.copy()
    want[1], want[2] = plain[1][:, ::-1, :], plain[2][:, ::-1, ::-1]
    assert same(T, run(T, src, [capi.augment_matrix([], 7, 9, 7, 9), v, hv], 7, 9, FILL), want)


def test_integer_shift_fills_what_leaves_the_source(T, small):
    src, plain = small
    shifts = [(1, 0), (-2, 1), (0, -3)]  # out[y][x] = plain[y + dy][x + dx]
    want = np.full_like(plain, 0.25)
    for b, (dx, dy) in enumerate(shifts):
        for y in range(7):
            for x in range(9):
                if 0 <= y + dy < 7 and 0 <= x + dx < 9:
                    want[b, :, y, x] = plain[b, :, y + dy, x + dx]
    assert (want == 0.25).any()
    assert same(T, run(T, src, [[1, 0, dx, 0, 1, dy] for dx, dy in shifts], 7, 9, 0.25), want)


def test_quarter_turns_equal_rot90(T):
    from cnn_amd import capi

    src = images(2, 6, 6, 12)
    plain = plain_stager_output(T, src).cpu().numpy()
    mats = [capi.augment_matrix([(capi.AUG_ROTATE, 90.0)], 6, 6, 6, 6), capi.augment_matrix([(capi.AUG_ROTATE, 270.0)], 6, 6, 6, 6)]
    want = np.stack([np.rot90(plain[0], 1, axes=(1, 2)), np.rot90(plain[1], 3, axes=(1, 2))])
    assert same(T, run(T, src, mats, 6, 6, FILL), want)


@pytest.mark.parametrize("H, W, shift_bytes", [(8, 12, 0), (5, 7, 0), (8, 12, 4)], ids=["quad_8x12", "tail_5x7", "unaligned_8x12"])
def test_resize_crop_and_rotation_equal_the_restatement(T, small, H, W, shift_bytes):
    """7x9 -> 8x12 (16-byte stores), -> 5x7 (W % 4 != 0) and -> 8x12 at a dst 4 bytes past a 16-byte boundary (per-pixel stores)"""
    from cnn_amd import capi

    src, _ = small
    A = capi
    resize = np.tile(capi.augment_matrix([], 7, 9, H, W), (3, 1))
    want, inside = R.augment(src, resize, H, W, FILL)
    assert inside.all() and not (want == FILL).any()  # the plain resize map produces no fill
    assert same(T, run(T, src, resize, H, W, FILL, shift_bytes), want)
    # crop (ratio >= 0.7) and rotation (<= 30 degrees) in three orders
    mats = np.stack([capi.augment_matrix([(A.AUG_CROP, 1, 1, 7, 5), (A.AUG_ROTATE, 30.0)], 7, 9, H, W),
                     capi.augment_matrix([(A.AUG_ROTATE, -20.0), (A.AUG_CROP, 0, 0, 8, 6)], 7, 9, H, W),
                     capi.augment_matrix([(A.AUG_ROTATE, 10.0), (A.AUG_HFLIP,), (A.AUG_CROP, 2, 1, 7, 6)], 7, 9, H, W)])
    want, inside = R.augment(src, mats, H, W, FILL)
    share = [1.0 - float(inside[b].mean()) for b in range(3)]
    assert max(share) < 0.5 and max(share) > 0.0, share  # asked of the reference before the kernel is looked at
    assert np.array_equal(want == FILL, np.broadcast_to(~inside[:, None], want.shape))
    assert same(T, run(T, src, mats, H, W, FILL, shift_bytes), want)


@pytest.mark.parametrize("Hs, Ws", [(1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 3)])
def test_tiny_sources(T, Hs, Ws):
    """sources of 3 ... 27 bytes per sample: below 8 bytes the kernel loads byte by byte, from 8 on its 4- and 8-byte loads must end
    inside the sample -- the last sample's last pixel sits at the end of the (guarded) buffer.  Whole-pixel and half-pixel maps."""
    from cnn_amd import capi

    src = images(2, Hs, Ws, 20 + 4 * Hs + Ws)
    plain = R.plain(src)
    ident = np.tile(capi.augment_matrix([], Hs, Ws, Hs, Ws), (2, 1))
    assert same(T, run(T, src, ident, Hs, Ws, FILL), plain)
    for H, W in ((4, 8), (5, 7)):
        mats = np.stack([capi.augment_matrix([], Hs, Ws, H, W), capi.augment_matrix([(capi.AUG_ROTATE, 180.0), (capi.AUG_ROTATE, 20.0)], Hs, Ws, H, W)])
        want, inside = R.augment(src, mats, H, W, FILL)
        assert inside[0].all()
        assert same(T, run(T, src, mats, H, W, FILL), want)


def test_a_map_outside_the_source_gives_fill_everywhere(T, small):
    src, _ = small
    mats = [[1, 0, 100, 0, 1, 0], [1, 0, 0, 0, 1, -8], [float("nan"), 0, 0, 0, 1, 0]]  # far right, one row above, not a number
    for H, W in ((7, 9), (8, 12)):
        want, inside = R.augment(src, mats, H, W, 0.25)
        assert not inside.any()
        got = run(T, src, mats, H, W, 0.25)
        assert same(T, got, want) and same(T, got, np.full((3, 3, H, W), 0.25, np.float32))


def test_workload_plane_with_sampled_matrices(T):
    """B = 4, 224x224 -> 224x224, hostapi.augment_params: the one case at the workload's plane size"""
    from cnn_amd import hostapi

    src = images(4, 224, 224, 13)
    mats = hostapi.augment_params(np.random.default_rng(5), 4, 224, 224, 224, 224, hflip=0.5, vflip=0.5, crop=1.0, rotate=1.0)
    want, inside = R.augment(src, mats, 224, 224, FILL)
    assert 0.0 < 1.0 - float(inside.mean()) < 0.5
    assert same(T, run(T, src, mats, 224, 224, FILL), want)


def test_bad_arguments_are_refused(T, small):
    from cnn_amd import capi

    src, _ = small
    s, m = T.from_numpy(src).cuda(), T.zeros((3, 6), device="cuda")
    for fill in (float("nan"), float("inf")):
        with pytest.raises(capi.CnnAmdError, match="fill"):
            capi.augment_u8(s, m, 7, 9, fill)
    with pytest.raises(capi.CnnAmdError, match="1..8192"):
        capi.augment_u8(s, m, 7, 8193)
    with pytest.raises(capi.CnnAmdError, match="1..8192"):
        capi.augment_u8(s, m, 0, 9, out=T.empty((3, 3, 7, 9), device="cuda"))  # (an empty tensor has no pointer: give it one)


def staged(T, st, src, mats=None, B=None, H=None, W=None):
    """one acquire / fill / submit / wait / copy out / release round of an augmenting stager"""
    from cnn_amd import capi

    host, slot = st.acquire()
    host[:] = src.reshape(-1)
    if mats is not None:
        st.matrices(slot)[:] = mats
    dev = st.submit(slot)
    st.wait(slot)
    got = T.empty((B, 3, H, W), device="cuda")
    capi.check(capi.load().cnn_memcpy_d2d(got.data_ptr(), dev, got.numel() * 4, capi._stream()), "cnn_memcpy_d2d")
    st.release(slot)
    T.cuda.synchronize()
    return got, slot


def test_augmenting_stager(T, small):
    from cnn_amd import capi

    src, plain = small
    st = capi.BatchStager(u8_shape=(3, 7, 9), depth=2, augment=True)
    # untouched matrices: the plain conversion
    got, slot0 = staged(T, st, src, None, 3, 7, 9)
    assert same(T, got, plain)
    # matrices written through matrices(slot): capi.augment_u8's bits, with the stager's fill
    st.set_fill(0.25)
    mats = np.stack([capi.augment_matrix([(capi.AUG_ROTATE, 25.0)], 7, 9, 7, 9), capi.augment_matrix([(capi.AUG_HFLIP,)], 7, 9, 7, 9),
                     np.array([1, 0, 3, 0, 1, -2], np.float32)])
    direct = run(T, src, mats, 7, 9, 0.25)
    assert (direct == 0.25).any()
    got, slot1 = staged(T, st, src, mats, 3, 7, 9)
    assert slot1 != slot0 and T.equal(got, direct)
    # the first slot again, after its release: acquire() preset its matrices, other bytes and maps give the new result
    src2 = images(3, 7, 9, 14)
    mats2 = mats[::-1].copy()
    got, slot2 = staged(T, st, src2, mats2, 3, 7, 9)
    assert slot2 == slot0 and T.equal(got, run(T, src2, mats2, 7, 9, 0.25))
    # and the second slot once more, untouched: the preset again, not the maps it carried before
    got, slot3 = staged(T, st, src2, None, 3, 7, 9)
    assert slot3 == slot1 and same(T, got, R.plain(src2))
    with pytest.raises(capi.CnnAmdError, match="fill"):
        st.set_fill(float("nan"))
    st.close()


def test_resizing_stager(T, small):
    """source 7x9, batch 8x12: untouched matrices are the plain resize map"""
    from cnn_amd import capi

    src, _ = small
    st = capi.BatchStager(u8_shape=(3, 8, 12), source_shape=(7, 9), depth=2)
    host, slot = st.acquire()
    assert host.size == 3 * 7 * 9 * 3
    assert np.array_equal(st.matrices(slot), np.tile(capi.augment_matrix([], 7, 9, 8, 12), (3, 1)))
    st.release(slot)
    got, _ = staged(T, st, src, None, 3, 8, 12)
    want, _ = R.augment(src, np.tile(capi.augment_matrix([], 7, 9, 8, 12), (3, 1)), 8, 12)
    assert same(T, got, want)
    st.close()


def test_matrices_and_set_fill_raise_on_the_other_stagers(T):
    from cnn_amd import capi

    for st in (capi.BatchStager(u8_shape=(3, 7, 9), depth=2), capi.BatchStager(3 * 3 * 7 * 9 * 4, depth=2)):
        with pytest.raises(capi.CnnAmdError, match="not an augmenting stager"):
            st.matrices(0)
        with pytest.raises(capi.CnnAmdError, match="not an augmenting stager"):
            st.set_fill(0.5)
        st.close()
