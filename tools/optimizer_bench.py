#!/usr/bin/env python3
"""The numbers of profiles/optimizer.md for the arena's step kernels, the clip and their cost inside a train step.
Method: HIP events around `launches` back-to-back calls (kernels) or `steps` back-to-back train_steps, every variant warmed up first,
the variants interleaved in one process, `rounds` rounds; median and minimum over the rounds.  Needs an MI355X.
usage: optimizer_bench.py [--rounds 15] [--out FILE.json] [--skip-steps]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnn_amd import capi, hostapi  # noqa: E402
from cnn_amd import stacks as S  # noqa: E402


def decay_ranges_of(layout):
    """the container's default decay policy: Conv2D / LinearLayer weights (tests/optim_ref.py has the full form)"""
    out, off = [], 0
    for e in layout:
        n = e["params"]
        if e["kind"] == "conv":
            out.append((off, off + n - e["Co"]))
        elif e["kind"] == "linear":
            out.append((off, off + n - e["n_out"]))
        off += n
    return out


def timed(T, fn, reps):
    a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def interleaved(T, variants, reps, rounds):
    """variants: {name: callable}; -> {name: (median us, min us, max us)}"""
    for fn in variants.values():
        timed(T, fn, max(2, reps // 4))
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(timed(T, fn, reps))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in samples.items()}


def kernel_table(T, rounds):
    layout = S.walk(S.vgg11(3))
    n = sum(e["params"] for e in layout)
    ranges = decay_ranges_of(layout)
    rs = np.random.RandomState(1)
    dev = lambda a: T.from_numpy(a).cuda()  # noqa: E731
    p = dev(rs.standard_normal(n).astype(np.float32))
    g = dev(rs.standard_normal(n).astype(np.float32) * np.float32(1e-3))
    vel, m, v, prev = (T.zeros(n, dtype=T.float32, device="cuda") for _ in range(4))
    lib = capi.load()
    table = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
    tab_p, nr = table.ctypes.data_as(capi.C.c_void_p), len(ranges)
    sgd = capi.SgdOptions(1e-3, 0.9, 5e-4, 0)
    adam = capi.AdamOptions(1e-3, 0.9, 0.999, 1e-8, 1e-2, 0, 7)
    adamw = capi.AdamOptions(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 7)
    ws_bytes = int(lib.cnn_clip_grad_norm_workspace_bytes(n))
    ws = T.empty(ws_bytes // 8, dtype=T.float64, device="cuda")
    stats = T.empty(2, dtype=T.float32, device="cuda")
    P, st = capi._ptr, capi._stream()

    def sgdm(prev_):
        return lambda: capi.check(lib.cnn_sgd_momentum_update(P(p), P(g), P(vel), n, capi.C.byref(sgd), 1.0, tab_p, None, nr, P(prev_), st), "sgdm")

    def adam_(opt, prev_, n_ranges=nr):
        return lambda: capi.check(lib.cnn_adam_update(P(p), P(g), P(m), P(v), n, capi.C.byref(opt), 1.0, tab_p, None, n_ranges, P(prev_), st), "adam")

    def clip(max_norm):
        return lambda: capi.check(lib.cnn_clip_grad_norm(P(g), n, max_norm, 1.0, P(ws), ws_bytes, P(stats), st), "clip")

    variants = {
        "sgdm_vec 9 ranges": (20, sgdm(None)),
        "sgdm_vec 9 ranges + previous": (24, sgdm(prev)),
        "adam_vec 9 ranges (L2)": (28, adam_(adam, None)),
        "adam_vec 9 ranges (L2) + previous": (32, adam_(adam, prev)),
        "adam_vec 9 ranges (decoupled) + previous": (32, adam_(adamw, prev)),
        "adam_vec 0 ranges": (28, adam_(adam, None, 0)),
        # 1e30 never engages: partial sums + finish + a scaling pass that returns at once (one read of the arena)
        "clip, coefficient 1 (3 launches)": (4, clip(1e30)),
    }
    res = interleaved(T, {k: fn for k, (_, fn) in variants.items()}, 20, rounds)
    rows = []
    for k, (bytes_per, _) in variants.items():
        med, lo, hi = res[k]
        rows.append(dict(kernel=k, bytes_per_element=bytes_per, us_median=med, us_min=lo, us_max=hi, tb_per_s=bytes_per * n / med * 1e-6))
    # a clip that engages rewrites the arena (12 B per element) and shrinks it every call: gradients refilled outside the timed window
    g0 = g.clone()
    samples = []
    for _ in range(rounds):
        g.copy_(g0)
        samples.append(timed(T, clip(1e-3), 1))
    rows.append(dict(kernel="clip, engaged (3 launches, one call per sample)", bytes_per_element=12, us_median=float(np.median(samples)),
                     us_min=float(np.min(samples)), us_max=float(np.max(samples)), tb_per_s=12 * n / float(np.median(samples)) * 1e-6))
    # the clip's three kernels one by one: the library's per-launch events (cnn_amd_kernel_timing_*, mode 1), 20 calls each
    breakdown = {}
    for label, max_norm in (("coefficient 1", 1e30), ("engaged", 1e-3)):
        g.copy_(g0)
        T.cuda.synchronize()
        capi.kernel_timing(1)
        for _ in range(20):
            clip(max_norm)()
        rep = capi.kernel_timing_report()
        capi.kernel_timing(0)
        breakdown[label] = {k.split("|")[0]: ms * 1e3 / cnt for k, (cnt, ms) in rep.items()}
    g.copy_(g0)
    return dict(n=n, ranges=nr, rows=rows, clip_breakdown_us=breakdown)


def step_table(T, rounds):
    out = []
    for B in (16, 256):
        x = T.from_numpy(np.random.RandomState(2).rand(B, 3, 224, 224).astype(np.float32)).cuda()
        labels = T.from_numpy((np.arange(B) % 3).astype(np.int32)).cuda()
        nets = {}
        for name in ("plain", "sgdm", "adam", "adamw", "plain + clip", "adam + clip"):
            net = hostapi.HostAlexNet(3)
            if name == "sgdm":
                net.set_optimizer(0.9, 5e-4)
            if name.startswith("adam"):
                net.set_adam(weight_decay=1e-2, decoupled=name == "adamw")
            if name.endswith("clip"):
                net.set_grad_clip(1.0)
            nets[name] = net
        res = interleaved(T, {k: (lambda net=net: net.train_step(x, labels, 1e-4)) for k, net in nets.items()}, 50, rounds)
        for net in nets.values():
            net.flush()
            net.close()
        out.append(dict(batch=B, us={k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    import torch as T

    assert T.cuda.is_available(), "optimizer_bench.py measures on the device: no GPU, no numbers"
    result = dict(kernels=kernel_table(T, args.rounds))
    if not args.skip_steps:
        result["steps"] = step_table(T, max(4, args.rounds * 4 // 5))
    k = result["kernels"]
    print(f"arena n = {k['n']}, {k['ranges']} decayed ranges")
    for r in k["rows"]:
        print(f"| `{r['kernel']}` | {r['bytes_per_element']} | {r['us_median']:.1f} | {r['us_min']:.1f} | {r['us_max']:.1f} | {r['tb_per_s']:.2f} |")
    for label, parts in k["clip_breakdown_us"].items():
        print(f"clip, {label}: " + ", ".join(f"{name} {us:.1f} us" for name, us in parts.items()))
    for s in result.get("steps", []):
        base = s["us"]["plain"]["median"]
        for name, v in s["us"].items():
            print(f"| {s['batch']} | {name} | {v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f}) | {v['median'] - base:+.1f} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
