#!/usr/bin/env python3
"""The numbers of profiles/evaluation.md: what evaluation on the device costs and what it saves.  Needs an MI355X.
(A) the kernel: one cnn_eval_accumulate launch (eval_accumulate) against the yardstick cnn_softmax_xent(probs = NULL)
    (softmax_xent_kernel: the same logits, the same per-sample arithmetic, and it also writes delta) at B = 256 with 3 and with 1000
    classes -- ONE process, the two kernels alternating run by run, five runs each; a run is HIP events around back-to-back launches.
    The bar: eval's median <= the yardstick's median + the yardstick's own max - min.
(B) the reference net's evaluation loop at B = 256 in images/s, every variant a fresh process, the variants alternating round by round:
      forward_host   what a commit without eval_step offers: forward_host under no_grad (host images: pack, upload, forward, one D2H of the
                     logits and a synchronise per batch) + NumPy argmax; run with --parent in the parent's tree and libraries
      eval_step      eval_begin, eval_step per batch on a device batch, ONE eval_result at the end
      eval_step_read the same with an eval_result behind every batch (what the read-back and the synchronise per batch cost)
    A sample is a host clock around a loop that ends in a synchronise.

usage: eval_bench.py [--parent DIR] [--rounds 5] [--out FILE.json]
  --parent DIR : a checkout of the PARENT commit with its libraries built (cnn_amd/lib/*.so); without it forward_host runs in this tree
  (worker)  --worker VARIANT --tree DIR : one process, prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys
import time

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


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def kernel_worker(T, capi):
    out = []
    for classes in (3, 1000):
        rs = np.random.RandomState(classes)
        logits = T.from_numpy((rs.standard_normal((B, classes)) * 3).astype(np.float32)).cuda()
        labels = T.from_numpy(rs.randint(0, classes, size=B).astype(np.int32)).cuda()
        state = T.zeros(capi.eval_state_bytes(classes), dtype=T.uint8, device="cuda")
        pred = T.empty(B, dtype=T.int32, device="cuda")
        delta = T.empty_like(logits)
        lib, s = capi.load(), capi._stream()
        P = capi._ptr
        fns = {"eval_accumulate": lambda: capi.check(lib.cnn_eval_accumulate(P(logits), P(labels), P(pred), P(state), B, classes, 1, s), "eval"),
               "softmax_xent_kernel": lambda: capi.check(lib.cnn_softmax_xent(P(logits), P(labels), None, P(delta), None, B, classes, s), "xent")}
        for fn in fns.values():
            timed(T, fn, 50)
        us = {k: [] for k in fns}
        for _ in range(5):  # (the two kernels alternate: a drift of the box shows in both)
            for k, fn in fns.items():
                us[k].append(timed(T, fn, 200))
        r = {k: spread(v) for k, v in us.items()}
        y = r["softmax_xent_kernel"]
        bar = y["median"] + (y["max"] - y["min"])
        out.append(dict(B=B, classes=classes, us=r, bar_us=bar, within_bar=bool(r["eval_accumulate"]["median"] <= bar)))
    print(json.dumps(out))


def worker(variant, tree):
    sys.path.insert(0, tree)
    import torch as T

    from cnn_amd import capi, hostapi

    assert T.cuda.is_available(), "eval_bench.py measures on the device: no GPU, no numbers"
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == os.path.abspath(tree), capi.__file__
    if variant == "kernel":
        return kernel_worker(T, capi)
    x = np.random.RandomState(2).rand(B, 3, 224, 224).astype(np.float32)
    labels = (np.arange(B) % 3).astype(np.int32)
    net = hostapi.HostAlexNet(3)
    net.set_params((np.random.RandomState(3).standard_normal(net.n_params) * 0.1).astype(np.float32))
    if variant == "forward_host":
        lib = hostapi.load()
        correct = [0]

        def loop(n):
            lib.cnnh_set_no_grad(1)
            for _ in range(n):
                correct[0] += int((np.argmax(net.forward_host(x), axis=1) == labels).sum())
            lib.cnnh_set_no_grad(0)

        per_sample = 5
    else:
        xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()

        def loop(n):
            net.eval_begin(1)
            for _ in range(n):
                net.eval_step(xd, ld)
                if variant == "eval_step_read":
                    net.eval_result()
            net.eval_result()

        assert variant in ("eval_step", "eval_step_read"), variant
        per_sample = 500
    loop(3)
    T.cuda.synchronize()
    rates = []
    for _ in range(4):
        t0 = time.perf_counter()
        loop(per_sample)
        T.cuda.synchronize()
        rates.append(B * per_sample / (time.perf_counter() - t0))
    net.close()
    print(json.dumps({"variant": variant, "tree": tree, "batches_per_sample": per_sample, "images_per_s": rates}))


def run_worker(variant, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--tree", tree]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:  # (a worker that failed ends the session: nothing more is started on the device)
        sys.exit(f"worker {variant} in {tree} failed with exit status {r.returncode}:\n{(r.stdout + r.stderr)[-3000:]}")
    print(f"  {variant} in {tree}: done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.tree))
    old = ("parent", os.path.abspath(args.parent)) if args.parent else ("this", ROOT)
    plan = [(old[0], old[1], "forward_host"), ("this", ROOT, "eval_step"), ("this", ROOT, "eval_step_read")]
    samples = {f"{t}:{v}": [] for t, _, v in plan}
    for _ in range(args.rounds):
        for t, tree, v in plan:
            samples[f"{t}:{v}"] += run_worker(v, tree)["images_per_s"]
    result = dict(batch=B, samples_per_variant=4 * args.rounds, images_per_s={k: spread(v) for k, v in samples.items()},
                  kernels=run_worker("kernel", ROOT))
    for k, v in result["images_per_s"].items():
        print(f"| {k} | {v['median']:.0f} ({v['min']:.0f} - {v['max']:.0f}) |")
    for shape in result["kernels"]:
        for k, v in shape["us"].items():
            print(f"| B={shape['B']} classes={shape['classes']} | {k} | {v['median']:.2f} ({v['min']:.2f} - {v['max']:.2f}) |")
        print(f"| B={shape['B']} classes={shape['classes']} | bar {shape['bar_us']:.2f} us | within: {shape['within_bar']} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
