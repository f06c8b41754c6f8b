"""No device needed: tests/resident_ref.py (the rule of the resident stager restated) against tests/augment_ref.py, and
hostapi.epoch_order, the sample order of one epoch over a resident dataset."""
import numpy as np
import pytest

from tests import augment_ref, photo_ref
from tests import resident_ref as RR


def test_identity_parameters_and_ascending_indices_are_the_plain_conversion():
    B, Hs, Ws = 5, 6, 7
    images = np.random.RandomState(21).randint(0, 256, size=(B, Hs, Ws, 3)).astype(np.uint8)
    labels = np.arange(B, dtype=np.int32) * 3
    mats, blocks = RR.identity_params(B, Hs, Ws, Hs, Ws)
    out, lab = RR.resident(images, labels, np.arange(B), mats, blocks, Hs, Ws)
    assert out.tobytes() == augment_ref.plain(images).tobytes()
    assert np.array_equal(lab, labels)


def test_an_absent_row_is_fill_under_the_box_and_carries_no_label():
    B, Hs, Ws = 3, 4, 8
    images = np.random.RandomState(22).randint(1, 256, size=(4, Hs, Ws, 3)).astype(np.uint8)
    labels = np.array([5, 6, 7, 8], np.int32)
    mats, blocks = RR.identity_params(B, Hs, Ws, Hs, Ws)
    blocks[1, 12:19] = (1, 1, 2, 2, 9.0, 8.0, 7.0)
    idx = np.array([3, -1, 0])
    out, lab = RR.resident(images, labels, idx, mats, blocks, Hs, Ws, fill=-2.0)
    assert np.array_equal(lab, [8, -1, 5])
    want = np.full((3, Hs, Ws), -2.0, np.float32)
    want[:, 1:3, 1:3] = np.array([9.0, 8.0, 7.0], np.float32)[:, None, None]
    assert out[1].tobytes() == want.tobytes()
    assert out[0].tobytes() == augment_ref.plain(images[3:4])[0].tobytes() and out[2].tobytes() == augment_ref.plain(images[0:1])[0].tobytes()
    # a zero image in the absent row's place is NOT the same thing: its pixels are inside
    zero = photo_ref.photo(np.zeros((1, Hs, Ws, 3), np.uint8), mats[:1], blocks[1:2], Hs, Ws, -2.0)[0]
    assert zero.tobytes() != out[1:2].tobytes()


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("batch", [1, 4, 256])
@pytest.mark.parametrize("n", [1, 7, 256, 1000])
def test_epoch_order(n, batch, world):
    from cnn_amd import hostapi

    ranks = [hostapi.epoch_order(n, batch, 5, 0, rank=r, world=world) for r in range(world)]
    for rows in ranks:
        assert rows.dtype == np.int32 and rows.ndim == 2 and rows.shape[1] == batch and rows.shape == ranks[0].shape
        flat = rows.reshape(-1)
        pad = flat == -1
        # -1 only at the tail of the last row
        assert not pad[:max(0, flat.size - batch)].any()
        assert not pad.any() or pad[np.argmax(pad):].all()
    everything = np.concatenate([rows.reshape(-1) for rows in ranks])
    assert sorted(everything[everything >= 0].tolist()) == list(range(n))  # every index exactly once over the ranks' rows
    assert ((everything >= -1) & (everything < n)).all()
    # rank r holds elements r, r + world, ... of ONE permutation
    perm = hostapi.epoch_order(n, 1, 5, 0).reshape(-1)
    for r, rows in enumerate(ranks):
        mine = rows.reshape(-1)
        assert np.array_equal(mine[mine >= 0], perm[r::world])
    # equal for equal (seed, epoch), another order in the next epoch and under another seed
    for r in range(world):
        assert np.array_equal(hostapi.epoch_order(n, batch, 5, 0, rank=r, world=world), ranks[r])
    if n > 1:
        assert not np.array_equal(hostapi.epoch_order(n, 1, 5, 1), hostapi.epoch_order(n, 1, 5, 0))
    # drop_last: no -1, full rows only, the same number on every rank, a prefix of the padded order
    for r in range(world):
        kept = hostapi.epoch_order(n, batch, 5, 0, drop_last=True, rank=r, world=world)
        assert kept.dtype == np.int32 and kept.shape == ((n // world) // batch, batch) and not (kept == -1).any()
        assert np.array_equal(kept, ranks[r][:kept.shape[0]])
    # shuffle=False: ascending
    plain = np.concatenate([hostapi.epoch_order(n, batch, 5, 3, shuffle=False, rank=r, world=world).reshape(-1) for r in range(world)])
    for r in range(world):
        mine = hostapi.epoch_order(n, batch, 5, 3, shuffle=False, rank=r, world=world).reshape(-1)
        assert np.array_equal(mine[mine >= 0], np.arange(n)[r::world])
    assert sorted(plain[plain >= 0].tolist()) == list(range(n))


def test_epoch_order_refuses_nonsense():
    from cnn_amd import capi, hostapi

    for kw in (dict(n=0, batch=1), dict(n=4, batch=0), dict(n=4, batch=2, rank=2, world=2), dict(n=4, batch=2, world=0)):
        with pytest.raises(capi.CnnAmdError):
            hostapi.epoch_order(seed=1, epoch=0, **kw)
