"""Stream order of the resident stager on a dataset with half-size levels (tests/stream_order.py is the harness).  Like the one-level
kind it takes no stream of its own: the consumer's ordering goes through cnn_batch_stager_wait / _release.  The wait proof of
tests/test_gpu_stream_order_resident.py, with the gather reading level 1."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import augment_ref
from tests import mip_ref
from tests import stream_order as SO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


@pytest.fixture
def H(T):
    h = SO.harness(T)
    try:
        yield h
    finally:
        h.finish()


def test_levelled_resident_stager_wait_orders_the_consumer_behind_the_gather(T, H):
    """wait(slot, S) in front of a consumer on S.  The stager's stream is out of a gate's reach, so the gather is made as long as a test
    can afford: B = 256 samples of 2048 x 2048, gathered from level 1 (1024 x 1024) into 1024 x 1024 through a half-pixel shift on that
    level, so that every pixel takes the four-tap route (3.2 GB written; measured at 0.39 ms for B = 64 against 0.18 ms of enqueue
    time, hence four times that batch).  The dataset holds two samples and every row of a batch reads the same one: the gather's
    time is its stores'.  The consumer -- a copy of the first sample's planes on S -- holds the new
    batch; one that did not wait would copy a slot in the middle of its gather.  Liveness as in
    tests/test_gpu_stream_order_resident.py: the host-side time from submit() to the queued consumer is at most a quarter of the
    gather's own time (timed once, submit to S idle), and the consumer is still pending when the host returns.  Where that cannot be
    established the case raises Unproven: it does not pass"""
    from cnn_amd import capi

    B, HW = 256, 1024
    rs = np.random.RandomState(8800)
    images = rs.randint(0, 256, size=(2, 2 * HW, 2 * HW, 3), dtype=np.uint8)
    ds = capi.ResidentDataset(2, 2 * HW, 2 * HW, levels=2)
    ds.write(0, images, [0, 1])
    stager = capi.BatchStager(depth=2, u8_shape=(B, HW, HW), resident=ds)
    old_idx = np.zeros(B, np.int32)
    new_idx = np.ones(B, np.int32)    # other bytes in the planes the consumer copies
    shift = np.tile(np.array([2, 0, 1.5, 0, 2, 1.5], np.float32), (B, 1))  # on level 1: [1, 0, 0.5, 0, 1, 0.5]
    level, on_level = mip_ref.choose(shift[0], 2)
    assert level == 1 and on_level.tolist() == [1, 0, 0.5, 0, 1, 0.5]
    new_out = augment_ref.augment(mip_ref.halve(images[1:2]), on_level[None, :], HW, HW)[0].reshape(-1)
    n = new_out.size
    try:
        with T.cuda.stream(H.S):
            for _ in range(2):  # both slots once, untimed: the first launch loads the kernel, and that is no gather time
                _, slot = stager.acquire()
                stager.indices(slot)[:] = old_idx
                stager.matrices(slot)[:] = shift
                stager.submit(slot)
                stager.wait(slot)
                stager.release(slot)
            _, slot = stager.acquire()
            stager.indices(slot)[:] = old_idx
            stager.matrices(slot)[:] = shift
            T.cuda.synchronize()
            t0 = time.perf_counter()
            stager.submit(slot)
            stager.wait(slot)
            H.S.synchronize()
            gather_ms = (time.perf_counter() - t0) * 1e3
            stager.release(slot)
            _, slot = stager.acquire()  # (the other slot: free)
            stager.indices(slot)[:] = new_idx
            stager.matrices(slot)[:] = shift
            seen = T.full((n,), 7.0, device="cuda")
            T.cuda.synchronize()
            t0 = time.perf_counter()
            dev_ptr = stager.submit(slot)
            stager.wait(slot)
            capi.check(capi.load().cnn_memcpy_d2d(capi._ptr(seen), C.c_void_p(dev_ptr), n * 4, capi._stream()), "cnn_memcpy_d2d")
            done = T.cuda.Event()
            done.record(H.S)
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            pending = not done.query()
            stager.release(slot)
        H.S.synchronize()
        assert (stager.levels(slot) == 1).all()
        H.enqueue_ms["stager wait u8_resident_levels"] = (enqueue_ms, gather_ms)
        print(f"stager wait u8_resident_levels: enqueue {enqueue_ms:.3f} ms, gather {gather_ms:.3f} ms, pending {pending}")
        if not (pending and 4 * enqueue_ms <= gather_ms):
            raise SO.Unproven(f"stager wait u8_resident_levels: the gather ({gather_ms:.3f} ms) was over before the consumer was queued "
                              f"({enqueue_ms:.3f} ms): nothing proven")
        assert seen.cpu().numpy().tobytes() == new_out.tobytes(), "the consumer behind wait() did not see its batch"
    finally:
        T.cuda.synchronize()
        stager.close()
        ds.close()
