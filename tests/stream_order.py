"""Gate harness of the stream-order tests (tests/test_gpu_stream_order_*.py): holds a stream-taking call to the order of its stream.

On a quiet device -- inputs finished long before the call, results read behind torch.cuda.synchronize() -- a kernel, memset or copy
on the wrong stream, a fork that does not wait for the caller's stream and a join that is missing all give the right numbers.  The
harness builds the opposite out of bounded, ordinary work:

  gate          a finite chain of the library's ReLU over a 256 MB tensor on one stream, followed by an event.  It ends by itself:
                nothing spins, nothing waits for the host.
  caller late   the call's input tensors hold a decoy (finite data of another seed), its workspaces a poison.  On the test stream S:
                the gate, the copies of the real inputs, the call, clones of its outputs.  The host waits with S.synchronize() only.
                Whatever the library queues outside S's order reads the decoy or the poison.
  helper late   the gate sits on a helper stream of the library (capi.side_stream()); S is free.  The clones on S follow the call
                and the join its contract names: a missing join clones the outputs' 7.0 fill.
  liveness      a gated run proves something only if the gate still ran while the library queued its work: gate_event.query() is
                asserted false right after the call returns (for a call that blocks the host by contract: right before it).  A run
                whose gate ended early is repeated once with a gate twice as long and must then be proven: no case is left unproven.

The reference of a gated run is never the code under test: a digest recorded from an earlier commit (tests/golden/*.json) or the
CPU oracle / a NumPy restatement at the bar of the call's own parity test.  Bit equality with the ungated run on S is asserted as
an extra.  Every case first runs once ungated on S, which also takes the first-call costs (module load, hipFuncSetAttribute) out of
the gated run's enqueue time."""
import hashlib
import math
import time

import numpy as np

from tests.util import REL_TOL, rel_err, uniform01

GATE_FLOATS = 64 << 20   # 256 MB in, 256 MB out per launch
# Length of a gate in milliseconds.  Measured on an MI355X (profiles/stream_order.md): one gate launch takes 0.10 ms (the harness
# times it with events when it is created and sizes every gate by that), the longest host-side enqueue of a single call in these
# files 0.35 ms.  Four times that is 1.4 ms; 20 ms leaves room for a host thread that is descheduled for a few milliseconds.  Cases
# that queue whole train steps behind one gate pass a longer one (gate_ms).
GATE_MS = 20.0
DECOY_FACTOR = 100.0     # reference(decoy) must differ from reference(real) by more than DECOY_FACTOR * REL_TOL

_harness = None


def harness(T):
    """the process-wide harness (one 512 MB gate buffer pair, one choice of S)"""
    global _harness
    if _harness is None:
        _harness = Harness(T)
    return _harness


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def decoy_of(real, seed):
    """finite data of another seed with the dtype and shape of `real` (NumPy): floats uniform in [-0.25, 0.75), integers permuted"""
    real = np.asarray(real)
    if real.dtype.kind == "f":
        return (uniform01(seed, real.shape) - np.float32(0.25)).astype(real.dtype)
    flat = real.reshape(-1)
    return np.ascontiguousarray(flat[np.random.RandomState(seed).permutation(flat.size)].reshape(real.shape))


def assert_decoy_differs(ref_real, ref_decoy, what):
    """a decoy that happens to give the right answer hides a failure: every output of the reference on the decoy inputs is further
    than DECOY_FACTOR * REL_TOL (tensor-normalised) from the reference on the real inputs"""
    assert sorted(ref_real) == sorted(ref_decoy), what
    for name in ref_real:
        e = rel_err(ref_decoy[name], ref_real[name])
        assert e > DECOY_FACTOR * REL_TOL, f"{what}: output {name} of the decoy is only {e:.3e} from the real one"


class Unproven(AssertionError):
    pass


class Result:
    """one case: `plain` (the ungated run on S) and `gated`, each {name: numpy} | int error code; enqueue_ms of the gated call"""

    def __init__(self, plain, gated, enqueue_ms):
        self.plain, self.gated, self.enqueue_ms = plain, gated, enqueue_ms

    def assert_same_bits_as_plain(self, what):
        if isinstance(self.plain, int) or isinstance(self.gated, int):
            assert self.plain == self.gated, (what, self.plain, self.gated)
            return
        assert sorted(self.plain) == sorted(self.gated), what
        for name, a in self.plain.items():
            assert a.tobytes() == self.gated[name].tobytes(), f"{what}: {name} differs between the gated and the ungated run"


class Harness:
    def __init__(self, T):
        from cnn_amd import capi

        self.T, self.capi = T, capi
        self.noise = T.rand((GATE_FLOATS,), device="cuda") - 0.5
        self.noise_out = T.empty_like(self.noise)
        self.probe = T.arange(1024, device="cuda", dtype=T.float32)
        T.cuda.synchronize()
        self.default = T.cuda.default_stream()
        self.side = capi.side_stream()
        self.keep = []          # every tensor of a case stays referenced until finish()
        self.enqueue_ms = {}    # case -> host-side enqueue time of the gated call
        self.repeated = []      # cases that needed the longer gate
        self.user_streams = 0
        self.launch_ms = self._time_gate_launch()
        self.S = self._pick_stream()
        self.S2 = self._new_stream()
        assert self.user_streams <= 3

    # ---- streams and gates -------------------------------------------------------------------------------------------------------
    def _new_stream(self):
        self.user_streams += 1
        return self.T.cuda.Stream()

    def _time_gate_launch(self):
        T = self.T
        for _ in range(3):
            self.capi.relu_forward(self.noise, self.noise_out)
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(16):
            self.capi.relu_forward(self.noise, self.noise_out)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 16

    def gate(self, stream, ms=None):
        """queues the gate on `stream`; -> the event behind it"""
        T = self.T
        launches = max(2, int(math.ceil((GATE_MS if ms is None else ms) / self.launch_ms)))
        with T.cuda.stream(stream):
            for _ in range(launches):
                self.capi.relu_forward(self.noise, self.noise_out)
            ev = T.cuda.Event()
            ev.record(stream)
        self.keep.append(ev)
        return ev

    def runs_beside(self, gated, other):
        """control, pure torch: with `gated` behind a gate, an op on `other` completes while the gate is live"""
        T = self.T
        ev = self.gate(gated)
        with T.cuda.stream(other):
            got = self.probe + 1
            done = T.cuda.Event()
            done.record(other)
        done.synchronize()
        live = not ev.query()
        T.cuda.synchronize()
        return live and bool(T.equal(got, self.probe + 1))

    def _pick_stream(self):
        """two streams may share a hardware queue, and a test stream that shares one with the default or the side stream proves
        nothing: S is the first of up to two candidates of torch's pool beside which both run"""
        tried = []
        for _ in range(2):
            s = self._new_stream()
            ok = (self.runs_beside(s, self.default), self.runs_beside(s, self.side), self.runs_beside(self.side, s))
            if all(ok):
                return s
            tried.append(ok)
        raise AssertionError(f"no test stream runs beside the default and the side stream (default, side, side gated): {tried}")

    def finish(self):
        """nothing stays gated behind a case, failed or not"""
        self.T.cuda.synchronize()
        self.keep.clear()

    # ---- the two placements ------------------------------------------------------------------------------------------------------
    def late(self, dst, seed, real=None, decoy=None):
        """(dst, real, decoy) for caller_late: `dst` is the device tensor the call reads, real (default: what dst holds now) arrives
        late, the decoy (default: decoy_of(real, seed)) is what dst holds until then"""
        T = self.T
        real = dst.clone() if real is None else real
        if decoy is not None:
            pass
        elif dst.dtype == T.uint8:  # (an opaque buffer, e.g. prepared filters: zero bytes are finite data)
            decoy = T.zeros_like(dst)
        else:
            decoy = T.from_numpy(decoy_of(real.cpu().numpy(), seed)).cuda()
        assert not T.equal(decoy, real)
        return dst, real, decoy

    def _outputs(self, call):
        """runs call() on the current stream: -> ({name: clone} | int error code, enqueue ms)"""
        t0 = time.perf_counter()
        try:
            out = call()
        except self.capi.CnnAmdError as e:
            import re

            out = int(re.search(r"failed with code (-?\d+)", str(e)).group(1))
        ms = (time.perf_counter() - t0) * 1e3
        if isinstance(out, int):
            return out, ms
        clones = {name: t.clone() for name, t in out.items()}
        self.keep.append((out, clones))
        return clones, ms

    def _scrub(self, plain):
        """What the ungated run left behind are the RIGHT bytes of the very call the gated run repeats: its outputs and their clones
        are overwritten with the poison (and stay referenced), or a block that goes back to the allocator could hand them to the
        gated run's outputs, where a reader that does not wait would find them in front of the 7.0 fill."""
        if isinstance(plain, int):
            return
        out, clones = self.keep[-1]
        with self.T.cuda.stream(self.S):
            for t in list(out.values()) + list(clones.values()):
                if t.is_contiguous():
                    t.view(-1).view(self.T.uint8).fill_(0xFF)
        self.S.synchronize()

    @staticmethod
    def _host(out):
        return out if isinstance(out, int) else {name: t.cpu().numpy() for name, t in out.items()}

    def _poison(self, late, poison, use_decoy):
        T = self.T
        with T.cuda.stream(self.S):
            for dst, real, decoy in late:
                dst.copy_(decoy if use_decoy else real)
            for p in poison:
                p.view(-1).view(T.uint8).fill_(0xFF)
        self.S.synchronize()

    def caller_late(self, name, late, call, poison=(), blocks=False, gate_ms=GATE_MS):
        """late: [(dst, real, decoy)] of self.late(); call() -> {name: output tensor} | int, run with S current; poison: workspaces
        and every buffer that outlives a call; blocks: the call waits for the device by contract (liveness is asserted in front of
        it); gate_ms: a longer gate for a case whose enqueue is long (at least four times it).  -> Result"""
        T, S = self.T, self.S
        self.keep.append((late, poison))
        self._poison(late, poison, use_decoy=False)
        with T.cuda.stream(S):
            plain, _ = self._outputs(call)
        S.synchronize()
        plain_dev, plain = plain, self._host(plain)
        self._scrub(plain_dev)
        for attempt in (0, 1):
            self._poison(late, poison, use_decoy=True)
            with T.cuda.stream(S):
                ev = self.gate(S, gate_ms)
                for dst, real, _ in late:
                    dst.copy_(real, non_blocking=True)
                live = not ev.query() if blocks else None
                gated, ms = self._outputs(call)
                if not blocks:
                    live = not ev.query()
            S.synchronize()
            if live:
                break
            T.cuda.synchronize()
            self.repeated.append(name)
            gate_ms *= 2
        if not live:
            raise Unproven(f"{name}: the gate ({gate_ms:.0f} ms) ended before the call was queued ({ms:.2f} ms): nothing proven")
        self.enqueue_ms[name] = ms
        return Result(plain, self._host(gated), ms)

    def helper_late(self, name, call, helper=None, poison=(), gate_ms=GATE_MS):
        """the gate sits on `helper` (default: the library's side stream), S is free; call() -> {name: output tensor}, run with S
        current, includes the join its contract names.  -> Result"""
        T, S = self.T, self.S
        helper = self.side if helper is None else helper
        self.keep.append(poison)
        self._poison((), poison, use_decoy=False)
        with T.cuda.stream(S):
            plain, _ = self._outputs(call)
        S.synchronize()
        T.cuda.synchronize()
        plain_dev, plain = plain, self._host(plain)
        self._scrub(plain_dev)
        for attempt in (0, 1):
            self._poison((), poison, use_decoy=False)
            ev = self.gate(helper, gate_ms)
            with T.cuda.stream(S):
                gated, ms = self._outputs(call)
                live = not ev.query()
            S.synchronize()
            if live:
                break
            T.cuda.synchronize()
            self.repeated.append(name)
            gate_ms *= 2
        if not live:
            raise Unproven(f"{name}: the helper gate ({gate_ms:.0f} ms) ended before the call was queued ({ms:.2f} ms): nothing proven")
        self.enqueue_ms[name] = ms
        return Result(plain, self._host(gated), ms)


# ---- which test runs which stream-taking export gated ------------------------------------------------------------------------------
_CONV = "tests/test_gpu_stream_order_conv.py::"
_LAYERS = "tests/test_gpu_stream_order_layers.py::test_layer_calls_caller_late"
_STREAMING = "tests/test_gpu_stream_order_streaming.py::test_streaming_cases_caller_late"
_PLUMBING = "tests/test_gpu_stream_order_plumbing.py::"
_CONTAINER = "tests/test_gpu_stream_order_container.py::test_container_on_a_caller_stream"
_PYNET = "tests/test_gpu_stream_order_pynet.py::test_python_driver_steps"


def _covered():
    table = {}
    for test, names in {
        _CONV + "test_conv_route_calls_caller_late": "conv2d_forward conv2d_forward_relu conv2d_backward_data conv2d_backward_data_relu conv2d_backward_weight",
        _CONV + "test_prepared_calls_caller_late": "conv2d_prepare_filters conv2d_forward_prepared conv2d_backward_data_prepared conv2d_backward_data_relu_prepared",
        _CONV + "test_fork_and_join": "conv2d_backward conv2d_backward_weight_side amd_side_stream_join amd_flush_reduces conv2d_backward_prepared "
                                      "conv2d_backward_prepared_relu conv2d_backward_pooled2_prepared",
        _CONV + "test_published_kernels": "amd_publish_next_kernel amd_wait_published",
        _CONV + "test_first_block_calls_caller_late": "conv2d_relu_maxpool2_forward conv2d_pool_mask_unpack conv2d_backward_weight_pooled2 conv2d_backward_data_pooled2",
        _CONV + "test_im2col_fallback_caller_late": "conv2d_forward_im2col conv2d_backward_weight_im2col conv2d_backward_data_im2col",
        _CONV + "test_tile_measurement_caller_late": "conv2d_autotune conv2d_autotune_ws",
        # (the deferred, pool-fused configuration of the Python driver: the prepared first-block forward, the one-launch weight
        # gradient + SGD step, the deferred data gradient from prepared filters)
        _PYNET: "conv2d_relu_maxpool2_forward_prepared conv2d_backward_weight_pooled2_sgd conv2d_backward_data_pooled2_prepared",
        # (the reference net's fused step tail, from its second step on)
        _CONTAINER: "conv2d_backward_weight_pooled2_sgd_keep",
        _STREAMING: "relu_forward relu_backward sgd_update sgd_update_keep sgd_momentum_update adam_update ema_update grad_accumulate arena_swap "
                    "clip_grad_norm dropout_forward dropout_backward",
        _LAYERS: "maxpool2d_forward maxpool2d_backward maxpool2d_backward_relu linear_forward linear_backward linear_backward_relu "
                 "batchnorm2d_forward batchnorm2d_forward_relu batchnorm2d_forward_relu_pool batchnorm2d_backward batchnorm2d_backward_pooled "
                 "batchnorm2d_partial_sums batchnorm2d_forward_from_sums batchnorm2d_forward_from_sums_relu batchnorm2d_backward_sums "
                 "batchnorm2d_backward_from_sums softmax_xent softmax_xent_soft linear_forward_softmax_xent linear_forward_softmax_xent_dx "
                 "linear_forward_softmax_xent_soft linear_forward_softmax_xent_soft_dx loss_from_terms soft_targets batch_mix eval_accumulate "
                 "eval_read grad_cam augment_u8",
        _PLUMBING + "test_layerwise_calls_caller_late": "segment_norms lamb_update lars_update",
        _PLUMBING + "test_plumbing_calls_caller_late": "memcpy_h2d memcpy_d2h memcpy_d2d memset_zero event_record stream_wait_event stream_wait_event_local",
        _PLUMBING + "test_one_rank_collectives_caller_late": "allreduce_grads comm_broadcast",
        _PLUMBING + "test_stager_wait_orders_the_consumer_behind_the_upload": "batch_stager_wait",
        _PLUMBING + "test_stager_release_orders_the_next_upload_behind_the_consumer": "batch_stager_release",
    }.items():
        for name in names.split():
            assert "cnn_" + name not in table, name
            table["cnn_" + name] = test
    return table


COVERED = _covered()
# exports that take a stream and queue no kernel, copy or memset on it
EXEMPT = {
    "cnn_amd_published_is_last": "a host-side question about the calling thread's bookkeeping; nothing is queued",
    "cnn_stream_synchronize": "waits on the host; nothing is queued",
    "cnn_stream_destroy": "destroys the stream it is given; nothing is queued",
    "cnn_amd_timing_span_begin": "a no-op unless kernel timing is on (off in every gated run); then it records a timing event, no work",
    "cnn_amd_timing_span_end": "a no-op unless kernel timing is on (off in every gated run); then it records a timing event, no work",
}
