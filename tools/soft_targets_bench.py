#!/usr/bin/env python3
"""The numbers of profiles/soft_targets.md: what label smoothing, mixup and CutMix cost.
(a) the reference net's default train_step at B = 256 on this commit and -- with --parent -- on the parent commit's build;
(b) the same step with set_label_smoothing(0.1): the step time and the head kernel's time (the library's kernel timer, every 4th
    launch bracketed) against the hard head's;
(c) cnn_batch_mix at 256 x 3 x 224 x 224 in MIXUP and in CUTMIX with a quarter-plane box against the yardstick gacc_vec_add (the
    existing 12 B-per-element streaming kernel) at the same n, the three alternating sample by sample in ONE process; bytes/s from
    the traffic model (mixup 12 B per element; CutMix 8 B; the yardstick 12 B); and train_step_mixed's step time.
Steps: HIP events around back-to-back steps, warmed up first; every variant is a fresh process, the variants alternate round by
round in ONE session; median, minimum and maximum over the samples.  Needs an MI355X.

usage: soft_targets_bench.py [--parent DIR] [--rounds 5] [--steps 200] [--out FILE.md]
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


def stat(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def kernel_worker(T, capi):
    shape = (B, 3, 224, 224)
    n = int(np.prod(shape))
    src = T.rand(shape, dtype=T.float32, device="cuda")
    dst = T.empty_like(src)
    mixup = capi.MixDesc(capi.MIX_MIXUP, 0.3, capi.PAIR_FLIP, 0, 0, 0, 0, 0)
    cutmix = capi.MixDesc(capi.MIX_CUTMIX, 0.75, capi.PAIR_FLIP, 0, 56, 168, 56, 168)  # a quarter of the plane
    fns = {"bmix_mixup_vec": (lambda: capi.batch_mix(mixup, src, dst), 12), "bmix_cutmix_vec": (lambda: capi.batch_mix(cutmix, src, dst), 8),
           "gacc_vec_add": (lambda: capi.grad_accumulate(dst, src, False), 12)}
    for fn, _ in fns.values():
        timed(T, fn, 10)
    us = {k: [] for k in fns}
    for _ in range(15):
        for k, (fn, _) in fns.items():
            us[k].append(timed(T, fn, 20))
    out = {k: dict(stat(us[k]), bytes_per_element=fns[k][1], gb_per_s=fns[k][1] * n / float(np.median(us[k])) * 1e-3) for k in fns}
    print(json.dumps(dict(n=n, kernels=out)))


def worker(variant, tree, steps):
    sys.path.insert(0, tree)
    import torch as T

    from cnn_amd import capi, hostapi

    assert T.cuda.is_available(), "soft_targets_bench.py measures on the device: no GPU, no numbers"
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == os.path.abspath(tree), capi.__file__
    if variant == "kernel":
        return kernel_worker(T, capi)
    x = T.from_numpy(np.random.RandomState(2).rand(B, 3, 224, 224).astype(np.float32)).cuda()
    labels = T.from_numpy((np.arange(B) % 3).astype(np.int32)).cuda()
    net = hostapi.HostAlexNet(3)
    step = lambda: net.train_step(x, labels, 1e-4)  # noqa: E731
    if variant == "smoothed":
        net.set_label_smoothing(0.1)
    elif variant in ("mixup", "cutmix"):
        net.set_label_smoothing(0.1)
        mix = (capi.MixDesc(capi.MIX_MIXUP, 0.3, capi.PAIR_FLIP, 0, 0, 0, 0, 0) if variant == "mixup" else
               capi.MixDesc(capi.MIX_CUTMIX, 0.75, capi.PAIR_FLIP, 0, 56, 168, 56, 168))
        step = lambda: net.train_step_mixed(x, labels, 1e-4, mix)  # noqa: E731
    else:
        assert variant == "default", variant
    timed(T, step, 20)
    us = [timed(T, step, steps // 4) for _ in range(4)]
    net.flush()
    T.cuda.synchronize()
    # the head kernel alone: every 4th launch of it bracketed by the library's timer
    capi.kernel_timing(2, "linear_fwd+softmax_xent", every=4)
    for _ in range(80):
        step()
    net.flush()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    head = {k.split("|")[0]: ms * 1e3 / cnt for k, (cnt, ms) in rep.items() if cnt}
    net.close()
    print(json.dumps({"variant": variant, "tree": tree, "us_per_step": us, "head_us": head}))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_targets.md"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    steps = max(4, args.steps // 4 * 4)
    if args.worker:
        return worker(args.worker, os.path.abspath(args.tree), steps)
    plan = [("this", v) for v in ("default", "smoothed", "mixup", "cutmix")]
    trees = {"this": ROOT}
    if args.parent:
        trees["parent"] = os.path.abspath(args.parent)
        plan.insert(1, ("parent", "default"))
    samples = {f"{t}:{v}": [] for t, v in plan}
    heads = {f"{t}:{v}": {} for t, v in plan}
    for _ in range(args.rounds):
        for t, v in plan:
            r = run_worker(v, trees[t], steps)
            samples[f"{t}:{v}"] += r["us_per_step"]
            for k, us in r["head_us"].items():
                heads[f"{t}:{v}"].setdefault(k, []).append(us)
    kernels = run_worker("kernel", ROOT, steps)
    lines = ["## Measured by tools/soft_targets_bench.py", "",
             f"Reference net, B = {B}, {steps // 4} back-to-back steps per sample, {4 * args.rounds} samples per variant, variants alternating "
             "round by round in one session, a fresh process each.", "", "| variant | us per step: median (min - max) | images/s at the median |",
             "|---|---|---|"]
    for k, v in samples.items():
        s = stat(v)
        lines.append(f"| {k} | {s['median']:.1f} ({s['min']:.1f} - {s['max']:.1f}) | {B / s['median'] * 1e6:.0f} |")
    lines += ["", "Head kernel inside the step (the library's kernel timer, every 4th launch bracketed):", "",
              "| variant | kernel | us: median (min - max) over the rounds |", "|---|---|---|"]
    for k, hs in heads.items():
        for name, v in hs.items():
            s = stat(v)
            lines.append(f"| {k} | {name} | {s['median']:.1f} ({s['min']:.1f} - {s['max']:.1f}) |")
    lines += ["", f"cnn_batch_mix at {B} x 3 x 224 x 224 (n = {kernels['n']}), 15 samples of 20 launches each, the three kernels alternating:", "",
              "| kernel | model B per element | us: median (min - max) | GB/s by the model | ratio to gacc_vec_add's GB/s |", "|---|---|---|---|---|"]
    yard = kernels["kernels"]["gacc_vec_add"]["gb_per_s"]
    for k, r in kernels["kernels"].items():
        lines.append(f"| {k} | {r['bytes_per_element']} | {r['median']:.1f} ({r['min']:.1f} - {r['max']:.1f}) | {r['gb_per_s']:.0f} | "
                     f"{r['gb_per_s'] / yard:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n" + text)


if __name__ == "__main__":
    main()
