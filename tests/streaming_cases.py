"""The cases and the record behind tests/golden/streaming.json: every entry point of cnn_amd/csrc/elementwise.hip whose kernels have the
streaming shape (stream_walk: float4 body, the <= 3 trailing elements in workgroup 0, a scalar kernel for unaligned pointers).

tests/golden/make_streaming.py and tests/test_gpu_streaming.py call the SAME function here (the mechanism of
tests/conv_route_cases.py, whose _logged is reused).  One record = one call on seeded inputs: its launch log and the SHA-256 of every
buffer the call may write.

Sizes: 1 and 3 (the scalar kernel although aligned), 4 (no tail), 7 (a tail of 3), 1027 (several waves and a tail) and one just past a
full grid (8 workgroups per compute unit), so that some lanes take a second grid-stride trip and a tail exists.  Every size runs with
all pointers 16-byte aligned and with the first one 4 bytes further (the scalar kernel)."""
import numpy as np

from tests.conv_route_cases import _logged

SMALL = [1, 3, 4, 7, 1027]
MANY = 64 + 6  # CNN_SGD_INLINE_RANGES + 6: the device-table instantiation


def past_a_full_grid(cus):
    return 4 * (8 * cus * 256) + 4 * 300 + 3


def table(name, n):
    """the range table `name` for n elements, None where it cannot be formed"""
    if name == "none":
        return []
    if name == "whole":
        return [(0, n)]
    if name == "cut":  # boundaries inside a float4, inside a wave, and a range that ends at n - 1 (inside the tail)
        if n >= 300:
            return [(1, 6), (250, 263), (n - 9, n - 1)]
        if n >= 7:
            return [(1, 3), (n - 2, n - 1)]
        return [(1, n - 1)] if n >= 3 else None
    assert name == "many"
    stride = n // MANY
    return [(k * stride + 1, k * stride + stride // 2 + 2) for k in range(MANY)] if stride >= 8 else None


def tables_at(n, names):
    """the names of `names` that can be formed at n (past SMALL without "whole": "cut" and "many" hold its case, a wave inside a range)"""
    return [t for t in names if table(t, n) is not None and (n in SMALL or t != "whole")]


ALL = ("none", "whole", "cut", "many")
# name -> (keyword arguments of capi.sgd_momentum_update, with `previous`, the tables it runs under)
SGDM = {
    "plain": (dict(lr=0.05), False, ("none",)),
    "m0_wd_prev": (dict(lr=0.05, weight_decay=0.01), True, ("whole", "cut", "many")),
    "mom_wd": (dict(lr=0.05, momentum=0.9, weight_decay=0.01), False, ALL),
    "nesterov_scaled_prev": (dict(lr=0.05, momentum=0.9, weight_decay=0.01, nesterov=True, grad_scale=0.5), True, ("cut",)),
}
ADAM = {
    "l2": (dict(lr=1e-3, weight_decay=0.01, step=3), False, ALL),
    "decoupled_prev": (dict(lr=1e-3, weight_decay=0.01, decoupled=True, step=3, grad_scale=0.5), True, ("cut", "many")),
}
EMA = {"avg": (0.999, ALL), "decay0": (0.0, ("cut",))}  # (the table none, and decay 0 under any table: the copy form)
SIMPLE = ["relu_fwd", "relu_bwd", "sgd", "sgd_keep", "gacc_first", "gacc_add", "aswap", "clip_engaged", "clip_idle", "dropout_fwd_train",
          "dropout_fwd_eval", "dropout_bwd"]


def case_list(sizes):
    """[(entry, variant, table name | None, n, offset)] -- only what can be formed: the record holds exactly these"""
    cases = []
    for n in sizes:
        for off in (0, 1):
            cases += [(e, "", None, n, off) for e in SIMPLE]
            for entry, variants in (("sgdm", SGDM), ("adam", ADAM)):
                for v, (_, _, names) in variants.items():
                    cases += [(entry, v, t, n, off) for t in tables_at(n, names)]
            for v, (_, names) in EMA.items():
                cases += [("ema", v, t, n, off) for t in tables_at(n, names)]
    return cases


def where(case):
    entry, variant, t, n, off = case
    return " ".join(x for x in (entry, variant, t and "table=" + t, f"n={n}", "aligned" if off == 0 else "+4") if x)


def _smallest_factor(n):
    return next((p for p in range(2, 65) if n % p == 0), n)


class _Inputs:
    """four seeded arrays of one size on the device; buf(k, off): a fresh copy of array k whose first element sits 4 * off bytes behind
    a 16-byte boundary"""

    def __init__(self, T, n):
        rs = np.random.RandomState(4200 + n % 1000)
        self.T, self.n = T, n
        self.dev = [T.from_numpy(rs.standard_normal(n).astype(np.float32)).cuda() for _ in range(4)]
        self.dev.append(self.dev[3] * self.dev[3])  # (a second moment: not negative)

    def buf(self, k, off=0):
        view = self.T.empty(self.n + 4, dtype=self.T.float32, device="cuda")[off:off + self.n]
        assert view.data_ptr() % 16 == 4 * off
        view.copy_(self.dev[k])
        return view


def _call(T, I, case):
    """-> the thunk of one case: runs the entry, returns {name: every buffer it may write}"""
    from cnn_amd import capi

    entry, variant, t, n, off = case
    lib = capi.load()
    ranges = table(t, n) if t else []

    def run():
        a = I.buf(0, off)
        if entry == "relu_fwd":
            return {"y": capi.relu_forward(I.buf(1), a)}
        if entry == "relu_bwd":
            return {"dy": capi.relu_backward(I.buf(1), a)}
        if entry == "sgd":
            return {"p": capi.sgd_update(a, I.buf(1), 0.05, 0.5)}
        if entry == "sgd_keep":
            prev = I.buf(2)
            capi.check(lib.cnn_sgd_update_keep(capi._ptr(a), capi._ptr(I.buf(1)), n, 0.05, 1.0, capi._ptr(prev), capi._stream()), "cnn_sgd_update_keep")
            return {"p": a, "previous": prev}
        if entry in ("gacc_first", "gacc_add"):
            return {"acc": capi.grad_accumulate(a, I.buf(1), entry == "gacc_first")}
        if entry == "aswap":
            b = I.buf(1)
            capi.arena_swap(a, b)
            return {"a": a, "b": b}
        if entry in ("clip_engaged", "clip_idle"):
            return {"g": a, "stats": capi.clip_grad_norm(a, 1e-3 if entry == "clip_engaged" else 1e9)}
        if entry.startswith("dropout"):
            C = _smallest_factor(n)
            shaped = a.view(1, C, n // C, 1)
            if entry == "dropout_bwd":
                return {"dy": capi.dropout_backward(shaped, 0.5)}
            return {"y": capi.dropout_forward(I.buf(1).view(1, C, n // C, 1), 0.5, entry == "dropout_fwd_train", shaped)}
        if entry == "sgdm":
            kw, with_prev, _ = SGDM[variant]
            out = {"p": a, "v": I.buf(2)}
            if with_prev:
                out["previous"] = I.buf(3)
            capi.sgd_momentum_update(a, I.buf(1), out["v"], decay_ranges=ranges, previous=out.get("previous"), **kw)
            return out
        if entry == "adam":
            kw, with_prev, _ = ADAM[variant]
            out = {"p": a, "m": I.buf(2), "v": I.buf(4)}
            if with_prev:
                out["previous"] = I.buf(3)
            capi.adam_update(a, I.buf(1), out["m"], out["v"], decay_ranges=ranges, previous=out.get("previous"), **kw)
            return out
        assert entry == "ema"
        return {"ema": capi.ema_update(a, I.buf(1), EMA[variant][0], ranges)}

    return run


def sizes_of(T):
    return SMALL + [past_a_full_grid(T.cuda.get_device_properties(T.cuda.current_device()).multi_processor_count)]


def streaming_record(T, repeats=1):
    """{where(case): {"log": ..., "sha": {...}}} over case_list(sizes_of(T)); repeats > 1 (the maker): every call runs that often --
    returns (record, [records whose digests did not repeat])"""
    rec, unstable = {}, []
    inputs = {}
    for case in case_list(sizes_of(T)):
        n = case[3]
        if n not in inputs:
            inputs.clear()  # (one size's inputs on the device at a time)
            inputs[n] = _Inputs(T, n)
        got = [_logged(T, _call(T, inputs[n], case)) for _ in range(repeats)]
        assert all(r["log"] == got[0]["log"] and "sha" in r for r in got), (where(case), got)
        if any(r["sha"] != got[0]["sha"] for r in got):
            unstable.append(where(case))
        assert where(case) not in rec
        rec[where(case)] = got[0]
    return rec, unstable
