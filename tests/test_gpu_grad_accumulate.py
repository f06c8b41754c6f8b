"""cnn_grad_accumulate (include/cnn_amd.h) on the device, through cnn_amd.capi: first = 1 is a copy of the bits, first = 0 one fp32 add
per element.  Every comparison is bit-exact against NumPy's float32 (where the reference is a NaN any NaN passes); the words are
compared on the device, the reference comes from the host once per size."""
import numpy as np
import pytest

from tests import guarded

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 4099, 111267, (1 << 24) + 5]


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch


def f32(*words):
    return np.array(words, np.uint32).view(np.float32)


# (acc, grads) pairs, as raw words: +-0, +-inf, quiet and signalling NaNs with payloads, denormals, and normal pairs whose sum is denormal
TINY = 0x00800000  # 2^-126, the smallest normal
PAIRS = [
    (0x00000000, 0x80000000), (0x80000000, 0x80000000), (0x80000000, 0x00000000), (0x3F800000, 0xBF800000),  # +0 + -0, -0 + -0, 1 + -1
    (0x7F800000, 0xFF800000), (0x7F800000, 0x7F800000), (0xFF800000, 0x3F800000), (0x3F800000, 0x7F800000),  # inf - inf = NaN, inf + inf, ...
    (0x7FC12345, 0x3F800000), (0x3F800000, 0xFFC00001), (0x7FA00001, 0x00000000), (0x00000000, 0x7F812345),  # NaN payloads either side
    (0x00000001, 0x00000001), (0x007FFFFF, 0x80000001), (0x00000001, 0x80000001), (0x807FFFFF, 0x807FFFFF),  # denormals (the last sums to a normal)
    (TINY + 0x400000, 0x80000000 | TINY), (0x80000000 | (TINY + 1), TINY), (TINY, 0x80000000 | 0x007FFFFF),   # normal + normal = denormal
    (0x7F7FFFFF, 0x7F7FFFFF), (0x00000000, 0x007FFFFF), (0x007FFFFF, 0x00000000),                              # overflow to inf, 0 + denormal
]


def make_inputs(n, seed):
    """-> (acc0, g): random normals with the special pairs planted at the tail (the <= 3 trailing elements and the float4 in front of
    them) and, where n allows, at the head and spread over the body"""
    rs = np.random.RandomState(seed)
    acc0, g = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    a, b = acc0.view(np.uint32), g.view(np.uint32)
    spots = [n - 1 - j for j in range(len(PAIRS))] + list(range(len(PAIRS))) + [(j * 4099 + 2048) % n for j in range(len(PAIRS))]
    for j in reversed(range(len(spots))):  # (small n: the tail placement is written last and wins)
        if 0 <= spots[j] < n:
            a[spots[j]], b[spots[j]] = PAIRS[(j + n) % len(PAIRS)]
    return acc0, g


def ref_add(a, b):
    with np.errstate(all="ignore"):
        out = a + b
    assert out.dtype == np.float32
    return out


class Want:
    """a host reference on the device: words to match, and where it is a NaN"""

    def __init__(self, T, host):
        self.host = host
        self.dev = T.from_numpy(host.view(np.int32).copy()).cuda()
        self.nan = T.from_numpy(np.isnan(host)).cuda()
        self.any_nan = bool(np.isnan(host).any())

    def mismatches(self, T, got_f32):
        """number of elements of the device tensor that are not the reference's words (any NaN where the reference is one)"""
        got_words = got_f32.view(T.int32)
        ok = got_words == self.dev
        if self.any_nan:
            ok = T.where(self.nan, T.isnan(got_f32), ok)
        return int((~ok).sum().item())


def one_gacc_kernel(rep, vec, first):
    names = [(k.split("|")[0], cnt) for k, (cnt, _) in rep.items()]
    return names == [("gacc_" + ("vec" if vec else "scalar") + ("_first" if first else "_add"), 1)], names


@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_numpy_bit_for_bit(T, n):
    """all 16 element offsets of (acc, grads), first = 1 and 0, acc inside a guarded allocation under both poisons: the result's words,
    the canaries, the untouched gradients, exactly one gacc_ launch per call (the float4 kernel only when both pointers are aligned and
    n >= 4).  Then three chained calls = (g1 + g2) + g3"""
    from cnn_amd import capi

    acc0, g = make_inputs(n, 7000 + n % 1000)
    want = {1: Want(T, g), 0: Want(T, ref_add(acc0, g))}
    assert want[0].any_nan or n < 5
    if n >= len(PAIRS):  # the inputs do hold what the test is about
        words = want[0].host.view(np.uint32)
        assert np.any((words & 0x7F800000) == 0) and np.any(words == 0x80000000) and np.any(words == 0x7F800000)
        assert np.any(((words & 0x7F800000) == 0) & ((words & 0x007FFFFF) != 0)), "a denormal sum"
    acc0_dev = T.from_numpy(acc0).cuda()
    g_words = T.from_numpy(g.view(np.int32).copy()).cuda()
    keep = []
    g_ops = [guarded.operand(g, guarded.POISONS[off % 2], keep, f"grads+{off}", shift_bytes=4 * off) for off in range(4)]
    problems = []
    for poison in guarded.POISONS:
        for a_off in range(4):
            acc = guarded.Scratch(4 * n, None, poison, f"acc+{a_off}", shift_bytes=4 * a_off)
            view = acc.view.view(T.float32)
            assert (view.data_ptr() % 16 == 0) == (a_off == 0)
            for g_off in range(4):
                gd = g_ops[g_off]
                assert (gd.data_ptr() % 16 == 0) == (g_off == 0)
                for first in (1, 0):
                    acc.refill()  # (first = 1: the accumulator holds the poison -- it is not read)
                    if not first:
                        view.copy_(acc0_dev)
                    T.cuda.synchronize()
                    capi.kernel_timing(1)
                    capi.grad_accumulate(view, gd, first)
                    rep = capi.kernel_timing_report()
                    capi.kernel_timing(0)
                    tag = f"n={n} poison={poison} acc+{a_off} grads+{g_off} first={first}"
                    bad = want[first].mismatches(T, view)
                    if bad:
                        problems.append(f"{tag}: {bad} element(s) differ from the reference")
                    ok, names = one_gacc_kernel(rep, a_off == 0 and g_off == 0 and n >= 4, first)
                    if not ok:
                        problems.append(f"{tag}: launches {names}")
                    if not acc.intact():
                        problems.append(f"{tag}: {acc.intact()}")
                    if not T.equal(gd.view(T.int32), g_words):
                        problems.append(f"{tag}: the gradients changed")
            del acc, view
    problems += guarded.check(keep)
    assert not problems, "\n  ".join(problems[:20])
    # a window of three: first = 1, then two adds, in the order a host loop would use
    rs = np.random.RandomState(n)
    g2, g3 = make_inputs(n, 8000 + n % 1000)
    g3 = g3[rs.permutation(n)]
    chained = Want(T, ref_add(ref_add(g, g2), g3))
    for a_off, g_off in ((0, 0), (1, 0), (0, 3)):
        acc = guarded.Scratch(4 * n, None, guarded.BYTES, "acc", shift_bytes=4 * a_off)
        view = acc.view.view(T.float32)
        for k, host in enumerate((g, g2, g3)):
            gd = guarded.operand(host, guarded.NAN, None, "grads", shift_bytes=4 * g_off)
            capi.grad_accumulate(view, gd, k == 0)
            T.cuda.synchronize()
        assert chained.mismatches(T, view) == 0 and acc.intact(), (n, a_off, g_off, str(acc.intact()))


def test_refusals_on_device_pointers(T):
    """null pointers, n == 0, acc == grads: a non-zero status and a message, nothing launched, nothing written"""
    from cnn_amd import capi

    lib = capi.load()
    host = np.arange(64, dtype=np.float32)
    a, b = T.from_numpy(host).cuda(), T.from_numpy(host + 1).cuda()
    T.cuda.synchronize()
    capi.kernel_timing(1)
    for args, word in (((None, capi._ptr(b), 64, 1), b"null"), ((capi._ptr(a), None, 64, 0), b"null"), ((capi._ptr(a), capi._ptr(b), 0, 1), b"n=0"),
                       ((capi._ptr(a), capi._ptr(a), 64, 0), b"same buffer")):
        assert lib.cnn_grad_accumulate(*args, capi._stream()) != 0
        msg = lib.cnn_amd_last_error()
        assert msg.startswith(b"cnn_grad_accumulate") and word in msg, msg
    with pytest.raises(capi.CnnAmdError, match="cnn_grad_accumulate"):
        capi.grad_accumulate(a, a, False)
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    assert rep == {}, rep
    assert np.array_equal(a.cpu().numpy(), host) and np.array_equal(b.cpu().numpy(), host + 1)
