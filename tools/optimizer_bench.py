#!/usr/bin/env python3
"""The numbers of profiles/optimizer.md for the arena's step kernels, the clip and their cost inside a train step.
Method: HIP events around `launches` back-to-back calls (kernels) or `steps` back-to-back train_steps, every variant warmed up first,
the variants interleaved in one process, `rounds` rounds; median and minimum over the rounds.  Needs an MI355X.
usage: optimizer_bench.py [--rounds 15] [--out FILE.json] [--skip-steps] [--layerwise]
--layerwise: the LAMB / LARS section instead (the segment norm, the passes of both updates beside adam_vec and sgdm_vec re-measured in
the same process, set_lamb / set_lars in a train step)."""
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


def segment_table_of(layout):
    """the container's default segment table (tests/lamb_ref.py has the full form): every tensor a segment, DECAY | ADAPT on weights"""
    bounds, flags, off = [0], [], 0
    for e in layout:
        n = e["params"]
        if e["kind"] in ("conv", "linear"):
            nb = e["Co"] if e["kind"] == "conv" else e["n_out"]
            parts = [(n - nb, capi.SEG_DECAY | capi.SEG_ADAPT), (nb, 0)]
        elif e["kind"] == "bn":
            parts = [(n // 4, 0)] * 4
        else:
            parts = []
        for cnt, fl in parts:
            off += cnt
            bounds.append(off)
            flags.append(fl)
    return np.array(bounds, np.uint32), np.array(flags, np.uint32)


def layerwise_kernel_table(T, rounds):
    """whole calls interleaved with adam_vec / sgdm_vec on the VGG-shaped arena, then every pass one by one from the library's per-launch
    events; the segment-norm call alone on this arena and on the reference net's"""
    lib = capi.load()
    P, st = capi._ptr, capi._stream()
    out = {}
    for arena, spec in (("vgg11", S.vgg11(3)), ("alexnet", S.alexnet(3))):
        layout = S.walk(spec)
        n = sum(e["params"] for e in layout)
        bounds, flags = segment_table_of(layout)
        ranges = decay_ranges_of(layout)
        rs = np.random.RandomState(1)
        dev = lambda a: T.from_numpy(a).cuda()  # noqa: E731
        p = dev(rs.standard_normal(n).astype(np.float32))
        g = dev(rs.standard_normal(n).astype(np.float32) * np.float32(1e-3))
        vel, m, v, upd, prev = (T.zeros(n, dtype=T.float32, device="cuda") for _ in range(5))
        norms = T.zeros(len(flags), dtype=T.float32, device="cuda")
        lw = capi.Layerwise(bounds, flags)
        table = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1))
        tab_p, nr = table.ctypes.data_as(capi.C.c_void_p), len(ranges)
        sgd = capi.SgdOptions(1e-5, 0.9, 5e-4, 0)
        adam = capi.AdamOptions(1e-5, 0.9, 0.999, 1e-8, 1e-2, 0, 7)
        lamb = capi.LambOptions(1e-5, 0.9, 0.999, 1e-6, 1e-2, 7)
        lars = capi.LarsOptions(1e-5, 0.9, 5e-4, 1e-3, 1e-8, 0)
        variants = {
            "adam_vec + previous": (32, lambda: capi.check(lib.cnn_adam_update(P(p), P(g), P(m), P(v), n, capi.C.byref(adam), 1.0, tab_p, None, nr,
                                                                               P(prev), st), "adam")),
            "sgdm_vec + previous": (24, lambda: capi.check(lib.cnn_sgd_momentum_update(P(p), P(g), P(vel), n, capi.C.byref(sgd), 1.0, tab_p, None, nr,
                                                                                       P(prev), st), "sgdm")),
            "cnn_lamb_update + previous (3 launches)": (28 + 16, lambda: capi.check(lib.cnn_lamb_update(lw.h, P(p), P(g), P(m), P(v), P(upd),
                                                                                                        capi.C.byref(lamb), 1.0, P(prev), st), "lamb")),
            "cnn_lars_update + previous (3 launches)": (8 + 24, lambda: capi.check(lib.cnn_lars_update(lw.h, P(p), P(g), P(vel), capi.C.byref(lars), 1.0,
                                                                                                       P(prev), st), "lars")),
            "cnn_segment_norms (2 launches)": (4, lambda: capi.check(lib.cnn_segment_norms(lw.h, P(g), P(norms), st), "norms")),
        }
        res = interleaved(T, {k: fn for k, (_, fn) in variants.items()}, 20, rounds)
        rows = []
        for k, (bytes_per, _) in variants.items():
            med, lo, hi = res[k]
            rows.append(dict(kernel=k, bytes_per_element=bytes_per, us_median=med, us_min=lo, us_max=hi, tb_per_s=bytes_per * n / med * 1e-6))
        # every pass one by one: the library's per-launch events (mode 1), `rounds` samples of 20 calls each, all variants in every sample
        per_pass = {}
        for _ in range(rounds):
            T.cuda.synchronize()
            capi.kernel_timing(1)
            for _ in range(20):
                for _, fn in variants.values():
                    fn()
            rep = capi.kernel_timing_report()
            capi.kernel_timing(0)
            for k, (cnt, ms) in rep.items():
                per_pass.setdefault(k.split("|")[0], []).append(ms * 1e3 / cnt)
        bytes_of = {"adam_vec": 32, "sgdm_vec": 24, "lamb_moments": 28, "lamb_apply": 16, "lars_norms": 8, "lars_apply": 24, "seg_norm_partial": 4}
        passes = []
        for name, samples in per_pass.items():
            med = float(np.median(samples))
            b = bytes_of.get(name)
            passes.append(dict(kernel=name, bytes_per_element=b, us_median=med, us_min=float(np.min(samples)), us_max=float(np.max(samples)),
                               tb_per_s=(b * n / med * 1e-6) if b else None))
        out[arena] = dict(n=n, segments=len(flags), rows=rows, passes=passes)
        lw.close()
    return out


def layerwise_step_table(T, rounds):
    out = []
    for B in (16, 256):
        x = T.from_numpy(np.random.RandomState(2).rand(B, 3, 224, 224).astype(np.float32)).cuda()
        labels = T.from_numpy((np.arange(B) % 3).astype(np.int32)).cuda()
        nets = {}
        for name in ("plain", "adam + clip", "lamb", "lars"):
            net = hostapi.HostAlexNet(3)
            if name == "adam + clip":
                net.set_adam(weight_decay=1e-2)
                net.set_grad_clip(1.0)
            if name == "lamb":
                net.set_lamb(weight_decay=1e-2)
            if name == "lars":
                net.set_lars(0.9, 5e-4)
            nets[name] = net
        res = interleaved(T, {k: (lambda net=net: net.train_step(x, labels, 1e-4)) for k, net in nets.items()}, 50, rounds)
        for net in nets.values():
            net.flush()
            net.close()
        out.append(dict(batch=B, us={k: dict(median=v[0], min=v[1], max=v[2]) for k, v in res.items()}))
    return out


def print_steps(steps):
    for s in steps:
        base = s["us"]["plain"]["median"]
        for name, v in s["us"].items():
            print(f"| {s['batch']} | {name} | {v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f}) | {v['median'] - base:+.1f} |")


def layerwise_main(T, args):
    result = dict(layerwise_kernels=layerwise_kernel_table(T, args.rounds))
    if not args.skip_steps:
        result["layerwise_steps"] = layerwise_step_table(T, max(4, args.rounds * 4 // 5))
    for arena, k in result["layerwise_kernels"].items():
        print(f"{arena}: arena n = {k['n']}, {k['segments']} segments")
        for r in k["rows"] + k["passes"]:
            rate = f"{r['tb_per_s']:.2f}" if r["tb_per_s"] else "-"
            print(f"| `{r['kernel']}` | {r['bytes_per_element'] or '-'} | {r['us_median']:.1f} | {r['us_min']:.1f} | {r['us_max']:.1f} | {rate} |")
    print_steps(result.get("layerwise_steps", []))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, "w"), indent=1)


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
    ap.add_argument("--layerwise", action="store_true")
    args = ap.parse_args()
    import torch as T

    assert T.cuda.is_available(), "optimizer_bench.py measures on the device: no GPU, no numbers"
    if args.layerwise:
        return layerwise_main(T, args)
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
