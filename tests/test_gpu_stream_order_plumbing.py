"""Stream order of the layer-wise optimizers and of the plumbing entry points (tests/stream_order.py is the harness):
cnn_segment_norms / cnn_lamb_update / cnn_lars_update on the smallest several-segment table of tests/test_gpu_layerwise.py, the copy
and memset helpers, cnn_event_record with both wait forms between S and a second stream, the one-rank collectives, and the batch
stagers: wait(slot, S) in front of a consumer on S, and the rule that a released slot is not overwritten before its consumer ran."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import stream_order as SO
from tests.lamb_ref import ref_lamb_moments, ref_lamb_step, ref_lars_step, ref_segment_norms
from tests.util import uniform_pm1

pytestmark = pytest.mark.gpu

N_SEG_TABLE = 5  # n = 5 under the table "seven" of tests/test_gpu_layerwise.py: five segments of one element, its smallest cut table


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


def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- layer-wise optimizers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["segment_norms", "lamb", "lars"])
def test_layerwise_calls_caller_late(T, H, entry):
    """parameters, gradient and state arrive late; the bars of tests/test_gpu_layerwise.py: every norm within one fp32 ulp of the fp64
    NumPy norm, everything behind the norms bit for bit with tests/lamb_ref.py evaluated from the device's own norms"""
    from cnn_amd import capi
    from tests.test_gpu_layerwise import LAMB, LARS, LR, make_data, make_flags, make_table, norms_close, same

    n = N_SEG_TABLE
    bounds = make_table("seven", n, 45)
    flags = make_flags("mixed", len(bounds) - 1)
    assert len(bounds) - 1 == 5
    p, (g,) = make_data(n, bounds, 46, 1)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lw = capi.Layerwise(bounds, flags)
    t = {"p": dev(T, p), "g": dev(T, g), "m": dev(T, m), "v": dev(T, v)}
    T.cuda.synchronize()
    late = [H.late(t[k], 8000 + i) for i, k in enumerate(("p", "g", "m"))]
    late.append(H.late(t["v"], 0, decoy=late[2][2] * late[2][2]))  # (a second moment: not negative)
    f7 = lambda k: T.full((k,), 7.0, device="cuda")
    wd, scale = 1e-2, 0.125
    try:
        if entry == "segment_norms":
            res = H.caller_late("segment_norms", late[:1], lambda: {"norms": lw.segment_norms(t["p"], f7(len(flags)))})
            norms_close(res.gated["norms"], ref_segment_norms(p, bounds), "stream order: segment norms")
        elif entry == "lamb":
            def call():
                u, prev = f7(n), f7(n)
                lw.lamb_update(t["p"], t["g"], t["m"], t["v"], u, LR, weight_decay=wd, step=1, grad_scale=scale, previous=prev, **LAMB)
                return {"p": t["p"], "m": t["m"], "v": t["v"], "update": u, "previous": prev}

            res = H.caller_late("lamb_update", late, call)
            wn, un, ratio = lw.stats()  # (of the latest call: the gated one)
            r, _, _ = ref_lamb_moments(p, g, m, v, bounds, flags, 1, weight_decay=wd, grad_scale=scale, **LAMB)
            norms_close(wn, ref_segment_norms(p, bounds), "stream order: lamb w_norm")
            norms_close(un, ref_segment_norms(r, bounds), "stream order: lamb u_norm")
            want_p, want_m, want_v, want_r, want_ratio = ref_lamb_step(p, g, m, v, bounds, flags, 1, LR, wn, un, weight_decay=wd, grad_scale=scale, **LAMB)
            assert same(ratio, want_ratio) and same(res.gated["update"], want_r)
            assert same(res.gated["m"], want_m) and same(res.gated["v"], want_v) and same(res.gated["p"], want_p)
            assert same(res.gated["previous"], p)
        else:
            def call():
                prev = f7(n)
                lw.lars_update(t["p"], t["g"], t["m"], LR, weight_decay=wd, grad_scale=scale, previous=prev, **LARS)
                return {"p": t["p"], "velocity": t["m"], "previous": prev}

            res = H.caller_late("lars_update", late[:3], call)
            wn, un, ratio = lw.stats()
            norms_close(wn, ref_segment_norms(p, bounds), "stream order: lars w_norm")
            gn = ref_segment_norms(g, bounds)
            norms_close(un, gn * np.float32(scale), "stream order: lars u_norm")
            want_p, want_v, want_gnt, want_ratio = ref_lars_step(p, g, m, bounds, flags, LR, wn, un, weight_decay=wd, grad_scale=scale,
                                                                 norm_is_scaled=True, **LARS)
            assert same(un, want_gnt) and same(ratio, want_ratio)
            assert same(res.gated["p"], want_p) and same(res.gated["velocity"], want_v) and same(res.gated["previous"], p)
        res.assert_same_bits_as_plain(entry)
    finally:
        T.cuda.synchronize()
        lw.close()


# ---- copies, memset, events ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["memcpy_d2d", "memcpy_d2h_h2d", "memset_zero", "event_wait", "event_wait_local"])
def test_plumbing_calls_caller_late(T, H, entry):
    """a device source that arrives late on S: the copy behind it holds the real bytes (device to device; device to pinned host and
    back); a memset on S lands behind the 7.0 fill in front of it; a second stream that waits through cnn_event_record +
    cnn_stream_wait_event[_local] for a gated producer on S sees its result"""
    from cnn_amd import capi

    lib, P, S_ = capi.load(), capi._ptr, capi._stream
    real = uniform_pm1(8100, (4099,))
    src = dev(T, real)
    T.cuda.synchronize()
    late = [H.late(src, 8101)]
    nbytes = src.numel() * 4
    pinned = T.full((src.numel(),), 7.0).pin_memory()
    event = C.c_void_p()
    capi.check(lib.cnn_event_create(C.byref(event)), "cnn_event_create")
    want = real
    out = T.empty_like(src)  # outside the call and poisoned in front of the gate: a reader on S2 that does not wait must not find
                             # there what the ungated run left

    def call():
        out.fill_(7.0)
        if entry == "memcpy_d2d":
            capi.check(lib.cnn_memcpy_d2d(P(out), P(src), nbytes, S_()), entry)
        elif entry == "memcpy_d2h_h2d":
            capi.check(lib.cnn_memcpy_d2h(C.c_void_p(pinned.data_ptr()), P(src), nbytes, S_()), "cnn_memcpy_d2h")
            capi.check(lib.cnn_memcpy_h2d(P(out), C.c_void_p(pinned.data_ptr()), nbytes, S_()), "cnn_memcpy_h2d")
        elif entry == "memset_zero":
            capi.check(lib.cnn_memset_zero(P(out), (src.numel() // 2) * 4, S_()), entry)
        else:
            capi.relu_forward(src, out)  # the producer on S
            capi.check(lib.cnn_event_record(event, S_()), "cnn_event_record")
            wait = lib.cnn_stream_wait_event if entry == "event_wait" else lib.cnn_stream_wait_event_local
            capi.check(wait(C.c_void_p(H.S2.cuda_stream), event), entry)
            with T.cuda.stream(H.S2):
                got = out.clone()
            T.cuda.current_stream().wait_stream(H.S2)
            return {"out": got}
        return {"out": out}

    try:
        res = H.caller_late(entry, late, call, poison=[out])
    finally:
        T.cuda.synchronize()
        lib.cnn_event_destroy(event)
    if entry == "memset_zero":
        want = np.concatenate([np.zeros(src.numel() // 2, np.float32), np.full(src.numel() - src.numel() // 2, 7.0, np.float32)])
    elif entry.startswith("event"):
        want = np.where(real >= 0, real, np.float32(0)).astype(np.float32)
    assert res.gated["out"].tobytes() == want.tobytes(), entry
    res.assert_same_bits_as_plain(entry)


@pytest.mark.parametrize("entry", ["allreduce", "broadcast"])
def test_one_rank_collectives_caller_late(T, H, entry):
    """cnn_allreduce_grads / cnn_comm_broadcast on a one-rank communicator are identities that go through RCCL on `stream`: a buffer
    that arrives late on S holds the real bytes behind the collective"""
    from cnn_amd import capi
    from cnn_amd.dp import RcclComm

    lib = capi.load()
    if not lib.cnn_comm_available():
        pytest.skip("librccl is not available")
    comm = RcclComm(None, 1, 0)
    real = uniform_pm1(8200, (100003,))
    buf = dev(T, real)
    T.cuda.synchronize()
    late = [H.late(buf, 8201)]

    def call():
        if entry == "allreduce":
            capi.check(lib.cnn_allreduce_grads(comm.handle, capi._ptr(buf), buf.numel(), capi._stream()), "cnn_allreduce_grads")
        else:
            capi.check(lib.cnn_comm_broadcast(comm.handle, capi._ptr(buf), buf.numel() * 4, 0, capi._stream()), "cnn_comm_broadcast")
        return {"buf": buf}

    try:
        res = H.caller_late("one-rank " + entry, late, call)
    finally:
        T.cuda.synchronize()
        comm.destroy()
    assert res.gated["buf"].tobytes() == real.tobytes()
    res.assert_same_bits_as_plain(entry)


# ---- batch stagers ---------------------------------------------------------------------------------------------------------------------
STAGERS = {"f32": dict(batch_bytes=4 * 3 * 64 * 64 * 4), "u8": dict(u8_shape=(4, 64, 64)), "u8_augment": dict(u8_shape=(4, 64, 64), augment=True)}


def _stager_batch(kind, seed):
    """(what the producer writes into the pinned slot, the fp32 batch the consumer must see)"""
    from tests import augment_ref

    if kind == "f32":
        a = uniform_pm1(seed, (4 * 3 * 64 * 64,))
        return a, a
    img = np.random.RandomState(seed).randint(0, 256, size=(4, 64, 64, 3)).astype(np.uint8)
    return img.reshape(-1), augment_ref.plain(img).reshape(-1)  # (an augmenting stager's preset map is the identity: the plain conversion)


@pytest.mark.parametrize("kind", sorted(STAGERS))
def test_stager_release_orders_the_next_upload_behind_the_consumer(T, H, kind):
    """wait(slot, S) in front of a consumer on S, and the reuse rule: a consumer on S sits behind a gate and still has to read slot 0;
    release(slot 0, S); the producer acquires its way round to slot 0 again and submits new bytes.  The consumer still sees the old
    batch (the release is an event on S behind the consumer: acquire() waits for it, as its contract says -- liveness is therefore
    asserted in front of that acquire)"""
    from cnn_amd import capi

    stager = capi.BatchStager(depth=2, **STAGERS[kind])
    old_in, old_out = _stager_batch(kind, 8300)
    new_in, new_out = _stager_batch(kind, 8301)
    n = old_out.size
    try:
        host, slot0 = stager.acquire()
        host[:] = old_in
        d0 = stager.submit(slot0)
        with T.cuda.stream(H.S):
            ev = H.gate(H.S)
            stager.wait(slot0)  # on S: the consumer below reads the slot behind its upload
            seen = T.full((n,), 7.0, device="cuda")
            capi.check(capi.load().cnn_memcpy_d2d(capi._ptr(seen), C.c_void_p(d0), n * 4, capi._stream()), "cnn_memcpy_d2d")
            stager.release(slot0)
        host, slot1 = stager.acquire()
        host[:] = new_in
        stager.submit(slot1)
        assert slot1 != slot0
        live = not ev.query()
        host, again = stager.acquire()  # blocks until S has passed the release of slot 0
        assert again == slot0
        host[:] = new_in
        d0_again = stager.submit(again)
        with T.cuda.stream(H.S):
            stager.wait(again)
            later = T.full((n,), 7.0, device="cuda")
            capi.check(capi.load().cnn_memcpy_d2d(capi._ptr(later), C.c_void_p(d0_again), n * 4, capi._stream()), "cnn_memcpy_d2d")
            stager.release(again)
        H.S.synchronize()
        assert live, "the gate ended before the slot was released and acquired again: nothing proven"
        assert d0_again == d0
        assert seen.cpu().numpy().tobytes() == old_out.astype(np.float32).tobytes(), "the consumer behind the gate saw other bytes than its batch"
        assert later.cpu().numpy().tobytes() == new_out.astype(np.float32).tobytes(), "the consumer of the re-used slot did not see the new batch"
    finally:
        T.cuda.synchronize()
        stager.close()


BIG_STAGERS = {"f32": dict(batch_bytes=16 * 1024 * 1024 * 4), "u8": dict(u8_shape=(8, 1024, 1024)), "u8_augment": dict(u8_shape=(8, 1024, 1024), augment=True)}


def _big_batch(kind, seed):
    from tests import augment_ref

    if kind == "f32":
        a = ((np.arange(16 * 1024 * 1024, dtype=np.int64) * 2654435761 + seed) % 2039).astype(np.float32) - np.float32(1000)
        return a, a
    img = np.random.RandomState(seed).randint(0, 256, size=(8, 1024, 1024, 3), dtype=np.uint8)
    return img.reshape(-1), augment_ref.plain(img).reshape(-1)


@pytest.mark.parametrize("kind", sorted(BIG_STAGERS))
def test_stager_wait_orders_the_consumer_behind_the_upload(T, H, kind):
    """wait(slot, S) in front of a consumer on S.  The upload runs on the stager's own stream, which no gate can reach, so the upload
    itself is made long: 64 MB of floats (25 MB of bytes and their conversion), about a millisecond, against a consumer that is queued
    some tens of microseconds behind submit().  The consumer -- a copy of the slot on S -- holds the new batch; a consumer that did
    not wait would copy a slot in the middle of its upload.  Liveness: the upload is timed once (submit to S idle), the host-side
    time from submit() to the queued consumer is at most a quarter of it, and the consumer is still pending when the host returns"""
    from cnn_amd import capi

    lib = capi.load()
    stager = capi.BatchStager(depth=2, **BIG_STAGERS[kind])
    old_in, _ = _big_batch(kind, 8400)
    new_in, new_out = _big_batch(kind, 8401)
    n = new_out.size
    try:
        with T.cuda.stream(H.S):
            host, slot = stager.acquire()
            host[:] = old_in
            T.cuda.synchronize()
            t0 = time.perf_counter()
            dev_ptr = stager.submit(slot)
            stager.wait(slot)
            H.S.synchronize()
            upload_ms = (time.perf_counter() - t0) * 1e3
            stager.release(slot)
            host, slot = stager.acquire()  # (the other slot: free)
            host[:] = new_in
            seen = T.full((n,), 7.0, device="cuda")
            T.cuda.synchronize()
            t0 = time.perf_counter()
            dev_ptr = stager.submit(slot)
            stager.wait(slot)
            capi.check(lib.cnn_memcpy_d2d(capi._ptr(seen), C.c_void_p(dev_ptr), n * 4, capi._stream()), "cnn_memcpy_d2d")
            done = T.cuda.Event()
            done.record(H.S)
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            pending = not done.query()
            stager.release(slot)
        H.S.synchronize()
        H.enqueue_ms[f"stager wait {kind}"] = (enqueue_ms, upload_ms)
        assert pending and 4 * enqueue_ms <= upload_ms, f"the upload ({upload_ms:.3f} ms) was over before the consumer was queued ({enqueue_ms:.3f} ms): nothing proven"
        assert seen.cpu().numpy().tobytes() == new_out.astype(np.float32).tobytes(), "the consumer behind wait() did not see its batch"
    finally:
        T.cuda.synchronize()
        stager.close()
