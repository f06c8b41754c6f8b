#!/usr/bin/env python3
"""The numbers of profiles/grad_accumulation.md: what a micro-batch of an accumulation window costs beside the same train step without it.
Method: HIP events around `steps` back-to-back train_steps of the reference net at B = 256, warmed up first; every variant is a fresh
process (the two libraries under comparison cannot share one), the variants alternate round by round in ONE session; median, minimum and
maximum over the rounds.  Needs an MI355X.

usage: grad_accumulation_bench.py [--parent DIR] [--rounds 5] [--steps 200] [--out FILE.json]
  --parent DIR : a checkout of the PARENT commit with its libraries built (cnn_amd/lib/*.so) -- its train_step with NO_FUSED_TAIL set is
                 the plain sequence without the accumulate launch (a), its default train_step the fused tail (b).  Without it the
                 same two variants are measured on this tree with k = 1 only.
  (worker)  --worker VARIANT --tree DIR : one process, prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K = 256, 4


def timed(T, fn, reps):
    a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def worker(variant, tree, steps):
    sys.path.insert(0, tree)
    import torch as T

    from cnn_amd import capi, hostapi
    from cnn_amd import stacks as S

    assert T.cuda.is_available(), "grad_accumulation_bench.py measures on the device: no GPU, no numbers"
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == os.path.abspath(tree), capi.__file__
    if variant == "kernel":  # (c) cnn_grad_accumulate alone on an arena of the VGG-shaped stack's size
        n = sum(e["params"] for e in S.walk(S.vgg11(3)))
        acc, g = T.zeros(n, dtype=T.float32, device="cuda"), T.full((n,), 1e-3, dtype=T.float32, device="cuda")
        out = {"n": n}
        for name, first, bytes_per in (("first", True, 8), ("add", False, 12)):
            fn = lambda first=first: capi.grad_accumulate(acc, g, first)  # noqa: E731
            timed(T, fn, 20)
            us = [timed(T, fn, 50) for _ in range(15)]
            out[name] = dict(bytes_per_element=bytes_per, us_median=float(np.median(us)), us_min=float(np.min(us)), us_max=float(np.max(us)),
                             gb_per_s=bytes_per * n / float(np.median(us)) * 1e-3)
        print(json.dumps(out))
        return
    x = T.from_numpy(np.random.RandomState(2).rand(B, 3, 224, 224).astype(np.float32)).cuda()
    labels = T.from_numpy((np.arange(B) % 3).astype(np.int32)).cuda()
    net = hostapi.HostAlexNet(3)
    if variant == "accumulate":
        net.set_grad_accumulation(K)
    elif variant == "no_fused_tail":
        capi.set_option("NO_FUSED_TAIL", "1")
    else:
        assert variant == "default", variant
    step = lambda: net.train_step(x, labels, 1e-4)  # noqa: E731
    timed(T, step, 5 * K)
    us = [timed(T, step, steps // 4) for _ in range(4)]  # (steps is a multiple of 4 * K: whole windows in every sample)
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
    steps = max(4 * K, args.steps // (4 * K) * (4 * K))
    if args.worker:
        return worker(args.worker, os.path.abspath(args.tree), steps)
    trees = {"this": ROOT}
    if args.parent:
        trees["parent"] = os.path.abspath(args.parent)
    plan = [("this", "accumulate")] + [(t, v) for t in reversed(sorted(trees)) for v in ("no_fused_tail", "default")]
    samples = {f"{t}:{v}": [] for t, v in plan}
    for _ in range(args.rounds):
        for t, v in plan:
            samples[f"{t}:{v}"] += run_worker(v, trees[t], steps)["us_per_step"]
    result = dict(batch=B, micro_steps=K, steps_per_sample=steps // 4, samples_per_variant=4 * args.rounds,
                  us_per_micro_batch={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in samples.items()},
                  kernel=run_worker("kernel", ROOT, steps))
    for k, v in result["us_per_micro_batch"].items():
        print(f"| {k} | {v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f}) |")
    kern = result["kernel"]
    for name in ("first", "add"):
        r = kern[name]
        print(f"| cnn_grad_accumulate first={int(name == 'first')} n={kern['n']} | {r['bytes_per_element']} | {r['us_median']:.1f} "
              f"({r['us_min']:.1f} - {r['us_max']:.1f}) | {r['gb_per_s']:.0f} GB/s |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
