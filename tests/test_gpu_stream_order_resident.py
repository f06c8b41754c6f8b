"""Stream order of the resident stager (tests/stream_order.py is the harness; the resident kind takes no stream of its own: the consumer's
ordering goes through cnn_batch_stager_wait / _release, as for the other kinds).  The reuse rule of
tests/test_gpu_stream_order_plumbing.py::test_stager_release_orders_the_next_upload_behind_the_consumer, and its wait proof at a shape
where one gather is long enough to prove anything."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import augment_ref
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


def _copy_out(T, capi, dev_ptr, n):
    out = T.full((n,), 7.0, device="cuda")
    capi.check(capi.load().cnn_memcpy_d2d(capi._ptr(out), C.c_void_p(dev_ptr), n * 4, capi._stream()), "cnn_memcpy_d2d")
    return out


def test_resident_stager_release_orders_the_next_gather_behind_the_consumer(T, H):
    """a gated consumer of slot 0 on S still sees its old batch after the producer has come round and resubmitted slot 0 with other
    indices; liveness is asserted in front of the acquire that has to wait for the release"""
    from cnn_amd import capi

    images = np.random.RandomState(8600).randint(0, 256, size=(8, 64, 64, 3)).astype(np.uint8)
    old_idx, new_idx = np.array([0, 1, 2, 3], np.int32), np.array([7, 6, 5, 4], np.int32)
    old_out, new_out = augment_ref.plain(images[old_idx]).reshape(-1), augment_ref.plain(images[new_idx]).reshape(-1)
    n = old_out.size
    ds = capi.ResidentDataset(8, 64, 64)
    ds.write(0, images, np.arange(8))
    stager = capi.BatchStager(depth=2, u8_shape=(4, 64, 64), resident=ds)
    try:
        _, slot0 = stager.acquire()
        stager.indices(slot0)[:] = old_idx
        d0 = stager.submit(slot0)
        with T.cuda.stream(H.S):
            ev = H.gate(H.S)
            stager.wait(slot0)  # on S: the consumer below reads the slot behind its gather
            seen = _copy_out(T, capi, d0, n)
            seen_lab = T.full((4,), 7, dtype=T.int32, device="cuda")
            capi.check(capi.load().cnn_memcpy_d2d(capi._ptr(seen_lab), C.c_void_p(stager.labels(slot0)), 16, capi._stream()), "cnn_memcpy_d2d")
            stager.release(slot0)
        _, slot1 = stager.acquire()
        stager.indices(slot1)[:] = new_idx
        stager.submit(slot1)
        assert slot1 != slot0
        live = not ev.query()
        _, again = stager.acquire()  # blocks until S has passed the release of slot 0
        assert again == slot0
        stager.indices(again)[:] = new_idx
        d0_again = stager.submit(again)
        with T.cuda.stream(H.S):
            stager.wait(again)
            later = _copy_out(T, capi, d0_again, n)
            stager.release(again)
        H.S.synchronize()
        assert live, "the gate ended before the slot was released and acquired again: nothing proven"
        assert d0_again == d0
        assert seen.cpu().numpy().tobytes() == old_out.tobytes(), "the consumer behind the gate saw other bytes than its batch"
        assert seen_lab.cpu().numpy().tolist() == [0, 1, 2, 3], "the consumer behind the gate saw other labels than its batch's"
        assert later.cpu().numpy().tobytes() == new_out.tobytes(), "the consumer of the re-used slot did not see the new batch"
    finally:
        T.cuda.synchronize()
        stager.close()
        ds.close()


def test_resident_stager_wait_orders_the_consumer_behind_the_gather(T, H):
    """wait(slot, S) in front of a consumer on S.  The stager's stream is out of a gate's reach and a gather is short, so it is made as
    long as a test can afford: B = 64 of 1024 x 1024 -> 1024 x 1024 through a half-pixel shift, so that every pixel takes the four-tap
    route (200 MB read, 800 MB written, measured at 0.3 ms on the one-tap route against 0.05 ms of enqueue time).  The consumer -- a
    copy of the first sample's planes on S -- holds the new batch; one that did not wait would copy a slot in the middle of its gather.
    Liveness as in tests/test_gpu_stream_order_plumbing.py: the host-side time from submit() to the queued consumer is at most a
    quarter of the gather's own time (timed once, submit to S idle), and the consumer is still pending when the host returns.  Where that
    cannot be established the case raises Unproven: it does not pass"""
    from cnn_amd import capi

    B, HW = 64, 1024
    rs = np.random.RandomState(8700)
    images = rs.randint(0, 256, size=(2, HW, HW, 3), dtype=np.uint8)
    ds = capi.ResidentDataset(B + 1, HW, HW)
    ds.write(0, images[0:1], [0])
    ds.write(B, images[1:2], [1])
    stager = capi.BatchStager(depth=2, u8_shape=(B, HW, HW), resident=ds)
    old_idx = np.arange(B, dtype=np.int32)            # sample 0 first
    new_idx = np.arange(B, 0, -1).astype(np.int32)    # sample B first: other bytes in the planes the consumer copies
    shift = np.tile(np.array([1, 0, 0.5, 0, 1, 0.5], np.float32), (B, 1))
    new_out = augment_ref.augment(images[1:2], shift[:1], HW, HW)[0].reshape(-1)
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
        H.enqueue_ms["stager wait u8_resident"] = (enqueue_ms, gather_ms)
        print(f"stager wait u8_resident: enqueue {enqueue_ms:.3f} ms, gather {gather_ms:.3f} ms, pending {pending}")
        if not (pending and 4 * enqueue_ms <= gather_ms):
            raise SO.Unproven(f"stager wait u8_resident: the gather ({gather_ms:.3f} ms) was over before the consumer was queued "
                              f"({enqueue_ms:.3f} ms): nothing proven")
        assert seen.cpu().numpy().tobytes() == new_out.tobytes(), "the consumer behind wait() did not see its batch"
    finally:
        T.cuda.synchronize()
        stager.close()
        ds.close()
