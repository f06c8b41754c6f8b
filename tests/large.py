"""Helpers of the large-tensor tests (tests/test_gpu_large_tensors.py) and of the pooled-domain BatchNorm
regression: batch sizes at a documented 32-bit limit, the restatement of a magic division without its correction step, the launch log,
device-side whole-tensor checks in sample chunks, memory accounting.  Nothing here asks the library where its limits are: the plan /
*_supported functions are the code under test."""
import numpy as np

GIB = 1 << 30


def batch_under(per_sample_elems, limit):
    """the largest B with B * per_sample_elems < limit ("over" is that B + 1)"""
    assert per_sample_elems > 0 and limit > per_sample_elems
    return (limit - 1) // per_sample_elems


def misdecoded_rows(H, W):
    """the elements hw of an H x W plane whose row umulhi(hw, ceil(2^32 / W)) -- a magic division WITHOUT its correction step -- is not
    hw // W (the quotient is then one too high), ascending"""
    magic = np.uint64(((1 << 32) + W - 1) // W)
    hw = np.arange(H * W, dtype=np.uint64)
    return np.nonzero(((hw * magic) >> np.uint64(32)) != hw // np.uint64(W))[0].astype(np.int64)


def misdecoded_slot_starts(H, W):
    """the subset of misdecoded_rows(H, W) that the pooled-domain BatchNorm kernels can show: they decode the FIRST element of an aligned
    4-element slot (hw % 4 == 0), and a row index one too high comes with a column W too low -- from an odd row that is the same pooled
    window again, from an EVEN row the window of the row above"""
    bad = misdecoded_rows(H, W)
    return bad[(bad % 4 == 0) & ((bad // W) % 2 == 0)]


def launch_log(capi, T, fn):
    """run fn() with the library's launch log on -> (fn's result, kernel names in first-launch order)"""
    capi.kernel_timing(1)
    try:
        out = fn()
        T.cuda.synchronize()
        names = [key.split("|")[0] for key in capi.kernel_timing_report()]
    finally:
        capi.kernel_timing(0)
    return out, names


def require_memory(T, footprint_bytes, what):
    """skip (with both numbers) only if the device has less free memory than the case's footprint + 4 GiB"""
    import pytest

    free, _total = T.cuda.mem_get_info()
    if free < footprint_bytes + 4 * GIB:
        pytest.skip(f"{what}: needs {footprint_bytes / GIB:.1f} GiB + 4 GiB, {free / GIB:.1f} GiB free on the device")
    T.cuda.reset_peak_memory_stats()


def release(T):
    """after the case's tensors went out of scope: hand the memory back (the card is shared)"""
    import gc

    gc.collect()
    T.cuda.empty_cache()


def sample_chunks(B, per_sample_elems, chunk_elems=1 << 27):
    """[i0, i1) sample ranges of at most ~chunk_elems elements: whole-tensor checks on the device without a second whole tensor"""
    step = max(1, chunk_elems // per_sample_elems)
    return [(i, min(B, i + step)) for i in range(0, B, step)]


def equal_in_chunks(T, B, per_sample_elems, got, want_of_range):
    """got[i0:i1] == want_of_range(i0, i1) bit for bit (T.equal) over the whole batch"""
    for i0, i1 in sample_chunks(B, per_sample_elems):
        if not T.equal(got[i0:i1], want_of_range(i0, i1)):
            return False
    return True


def fill_uniform(T, t, gen, lo, hi, chunk_elems=1 << 28):
    """t <- uniform [lo, hi) in place, in flat chunks (no whole-tensor temporary)"""
    flat = t.view(-1)
    for i in range(0, flat.numel(), chunk_elems):
        flat[i : i + chunk_elems].uniform_(lo, hi, generator=gen)
    return t


REPORT = []  # one dict per large case: what ran on which side of its limit, kernels, peak memory, seconds


def report(**kw):
    REPORT.append(kw)
    print("LARGE " + " ".join(f"{k}={v}" for k, v in kw.items()), flush=True)
