#!/usr/bin/env python3
"""The numbers of profiles/ema.md: what the parameter average costs.
(a) kernels: one ema_vec launch (12 B per element), one aswap_vec launch (16 B per element) and, as the yardstick, one gacc_vec_add
    launch (12 B per element) at three arena sizes -- the reference net's, the VGG-shaped stack's, the ResNet-shaped stack's -- in ONE
    process, the three kernels alternating sample by sample.  ema_vec runs with the table the container builds for that net
    (everything but BatchNorm2D's moving statistics).
(b) the reference net's train_step at B = 256 with the average off and on, and -- with --parent -- the parent commit's default step:
    HIP events around back-to-back train_steps, warmed up first; every variant is a fresh process, the variants alternate round by
    round in ONE session; median, minimum and maximum over the samples.  Needs an MI355X.

(c) where ema_vec's time goes: at the ResNet-shaped stack's n, through the bare C entries (no Python wrapper between the launches):
    gacc_vec_add, the copy form, and ema_vec with tables of 1, the net's 18, 64 (the largest inline table) and 70 ranges (the device
    table), alternating.

usage: ema_bench.py [--parent DIR] [--rounds 5] [--steps 200] [--out FILE.json]
  --parent DIR : a checkout of the PARENT commit with its libraries built (cnn_amd/lib/*.so)
  (worker)  --worker VARIANT --tree DIR : one process, prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 256


def timed(T, fn, reps):
    a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def averaged_ranges(layout):
    """the table Sequential::set_ema builds: every layer's parameters but the second half of a BatchNorm2D block, neighbours merged"""
    out, off = [], 0
    for e in layout:
        n = e["params"]
        keep = n // 2 if e["kind"] == "bn" else n
        if keep:
            if out and out[-1][1] == off:
                out[-1] = (out[-1][0], off + keep)
            else:
                out.append((off, off + keep))
        off += n
    return out


def summary(us, bytes_per, n):
    med = float(np.median(us))
    return dict(bytes_per_element=bytes_per, us_median=med, us_min=float(np.min(us)), us_max=float(np.max(us)), gb_per_s=bytes_per * n / med * 1e-3)


def kernel_worker(T, capi, S):
    out = []
    for name, spec in (("alexnet", S.alexnet(3)), ("vgg11", S.vgg11(3)), ("resnet18", S.resnet18(3))):
        layout = S.walk(spec)
        n = sum(e["params"] for e in layout)
        ranges = averaged_ranges(layout)
        assert len(ranges) <= capi.SGD_INLINE_RANGES
        ema, p = T.zeros(n, dtype=T.float32, device="cuda"), T.full((n,), 1e-3, dtype=T.float32, device="cuda")
        fns = {"ema_vec": (lambda: capi.ema_update(ema, p, 0.999, ranges), 12), "aswap_vec": (lambda: capi.arena_swap(ema, p), 16),
               "gacc_vec_add": (lambda: capi.grad_accumulate(ema, p, False), 12)}
        for fn, _ in fns.values():
            timed(T, fn, 20)
        us = {k: [] for k in fns}
        for _ in range(15):  # (the three kernels alternate: a drift of the box shows in all of them)
            for k, (fn, _) in fns.items():
                us[k].append(timed(T, fn, 50))
        out.append(dict(net=name, n=n, ranges=len(ranges), kernels={k: summary(us[k], fns[k][1], n) for k in fns}))
    print(json.dumps(out))


def cut_ranges(n, count):
    """`count` ranges of equal length with gaps between them, begins and ends inside float4s"""
    stride = n // count
    return [(k * stride + 1, k * stride + stride // 2 + 2) for k in range(count)]


def table_worker(T, capi, S):
    import ctypes as C

    layout = S.walk(S.resnet18(3))
    n = sum(e["params"] for e in layout)
    ema, p = T.zeros(n, dtype=T.float32, device="cuda"), T.full((n,), 1e-3, dtype=T.float32, device="cuda")
    lib, e, q, s = capi.load(), capi._ptr(ema), capi._ptr(p), capi._stream()
    keep = []

    def raw_ema(ranges, decay=0.999):
        t = np.ascontiguousarray(np.asarray(ranges, np.uint32).reshape(-1, 2))
        dev = T.from_numpy(t.view(np.int32).reshape(-1)).cuda() if len(ranges) > capi.SGD_INLINE_RANGES else None
        keep.append((t, dev))
        tp, d, nr = t.ctypes.data_as(C.c_void_p), capi._ptr(dev), len(ranges)
        return lambda: capi.check(lib.cnn_ema_update(e, q, n, decay, tp, d, nr, s), "cnn_ema_update")

    fns = {"gacc_vec_add": lambda: capi.check(lib.cnn_grad_accumulate(e, q, n, 0, s), "cnn_grad_accumulate"),
           "ema_vec_copy (decay 0)": raw_ema([(0, n)], 0.0),
           "ema_vec, 1 range [0, n)": raw_ema([(0, n)]),
           "ema_vec, the net's 18 ranges": raw_ema(averaged_ranges(layout)),
           "ema_vec, 64 ranges (inline)": raw_ema(cut_ranges(n, 64)),
           "ema_vec, 70 ranges (device table)": raw_ema(cut_ranges(n, 70))}
    for fn in fns.values():
        timed(T, fn, 20)
    us = {k: [] for k in fns}
    for _ in range(15):
        for k, fn in fns.items():
            us[k].append(timed(T, fn, 50))
    print(json.dumps(dict(n=n, us={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in us.items()})))


def worker(variant, tree, steps):
    sys.path.insert(0, tree)
    import torch as T

    from cnn_amd import capi, hostapi
    from cnn_amd import stacks as S

    assert T.cuda.is_available(), "ema_bench.py measures on the device: no GPU, no numbers"
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == os.path.abspath(tree), capi.__file__
    if variant == "kernel":
        return kernel_worker(T, capi, S)
    if variant == "table":
        return table_worker(T, capi, S)
    x = T.from_numpy(np.random.RandomState(2).rand(B, 3, 224, 224).astype(np.float32)).cuda()
    labels = T.from_numpy((np.arange(B) % 3).astype(np.int32)).cuda()
    net = hostapi.HostAlexNet(3)
    if variant == "ema_on":
        net.set_ema(0.999, warmup=True)
    elif variant == "ema_off_again":
        net.set_ema(0.999)
        net.set_ema(0)
    elif variant == "no_fused_tail":
        capi.set_option("NO_FUSED_TAIL", "1")
    else:
        assert variant == "default", variant
    step = lambda: net.train_step(x, labels, 1e-4)  # noqa: E731
    timed(T, step, 20)
    us = [timed(T, step, steps // 4) for _ in range(4)]
    net.flush()
    T.cuda.synchronize()
    net.close()
    print(json.dumps({"variant": variant, "tree": tree, "us_per_step": us}))


def run_worker(variant, tree, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--tree", tree, "--steps", str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:  # (a worker that failed ends the session: nothing more is started on the device)
        sys.exit(f"worker {variant} in {tree} failed with exit status {r.returncode}:\n{(r.stdout + r.stderr)[-3000:]}")
    print(f"  {variant} in {tree}: done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    steps = max(4, args.steps // 4 * 4)
    if args.worker:
        return worker(args.worker, os.path.abspath(args.tree), steps)
    plan = [("this", v) for v in ("ema_on", "default", "ema_off_again", "no_fused_tail")]
    trees = {"this": ROOT}
    if args.parent:
        trees["parent"] = os.path.abspath(args.parent)
        plan.append(("parent", "default"))
    samples = {f"{t}:{v}": [] for t, v in plan}
    for _ in range(args.rounds):
        for t, v in plan:
            samples[f"{t}:{v}"] += run_worker(v, trees[t], steps)["us_per_step"]
    result = dict(batch=B, steps_per_sample=steps // 4, samples_per_variant=4 * args.rounds,
                  us_per_step={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in samples.items()},
                  kernels=run_worker("kernel", ROOT, steps), table=run_worker("table", ROOT, steps))
    for k, v in result["us_per_step"].items():
        print(f"| {k} | {v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f}) |")
    for net in result["kernels"]:
        for k, r in net["kernels"].items():
            print(f"| {net['net']} n={net['n']} ranges={net['ranges']} | {k} | {r['bytes_per_element']} | {r['us_median']:.2f} "
                  f"({r['us_min']:.2f} - {r['us_max']:.2f}) | {r['gb_per_s']:.0f} GB/s |")
    for k, v in result["table"]["us"].items():
        print(f"| n={result['table']['n']} | {k} | {v['median']:.2f} ({v['min']:.2f} - {v['max']:.2f}) |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
