#!/usr/bin/env python3
"""The numbers of profiles/resident_dataset.md: what gathering batches out of a device-resident dataset costs and buys.  Needs an MI355X.
The method is tools/augment_bench.py's: fresh processes, the variants alternating, medians with minimum and maximum.
(A) the launch alone, B = 256, 224 x 224 -> 224 x 224: augment_u8_photo (the host-fed photo stager's kernel; with --parent also in the
    parent's tree, the two trees alternating process by process) against augment_u8_resident with idx = arange(256) out of a 256-sample
    dataset, and with 256 indices drawn from a 10 000-sample dataset (1.5 GB), another draw every launch; each with the blocks acquire() presets and with
    hostapi.augment_params + photo_params, ImageNet's mean / std and the clamp.  The clock is the library's own per-launch HIP events
    (cnn_amd_kernel_timing_enable) around each launch, where it runs in use: on the stager's stream.  One process runs every variant,
    alternating run by run, five runs each; a run is the mean over 20 launches.
(B) the staged training loop of the reference net at B = 256 in images/s, every variant a fresh process, alternating round by round:
      u8        the plain u8 stager (acquire, submit, wait, train step, release)
      photo     the photo stager with augment_params matrices and photo_params blocks copied into the slot every step, mean / std, clamp
      resident  HostNet.train_epoch_resident over a 4096-sample dataset in hostapi.epoch_order's shuffled order, the same matrices and blocks
      resident_depth3  the same with three slots instead of two: with one batch of look-ahead and two slots, the acquire() for batch i + 1
                waits on the host for step i - 1 to finish, and step i is queued only behind that wait
      resident_gather_only  the same loop without the train step: what the host and the stager's stream can deliver on their own
      unstaged  the step alone on a batch that is already on the device (bench.py's headline)
    A sample is a host clock around a loop of steps that ends in a synchronise.  The requirement: resident above photo's maximum.

usage: resident_bench.py [--parent DIR] [--rounds 3] [--kernel-rounds 2] [--legs kernel,loop] [--out FILE.json] [--md FILE.md]
  (worker)  --worker VARIANT --tree DIR : one process, prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, HW = 256, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LOOP_N, KERNEL_N = 4096, 10000
LOOP_VARIANTS = ("u8", "photo", "resident", "resident_depth3", "resident_gather_only", "unstaged")


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def filled_dataset(capi, n, seed):
    """n samples of HW x HW: one random block of 256 samples written again and again (what a gather costs depends on where its bytes lie,
    not on what they are), labels i % 3"""
    block = np.random.RandomState(seed).randint(0, 256, size=(256, HW, HW, 3), dtype=np.uint8)
    ds = capi.ResidentDataset(n, HW, HW)
    for first in range(0, n, 256):
        count = min(256, n - first)
        ds.write(first, block[:count], (np.arange(first, first + count) % 3).astype(np.int32))
    return ds, block


def kernel_worker(T, capi, hostapi):
    params = hostapi.augment_params(np.random.default_rng(2), B, HW, HW, HW, HW)
    blocks = hostapi.photo_params(np.random.default_rng(3), B, HW, HW)
    has_resident = hasattr(capi, "ResidentDataset")  # (the parent's tree has none)
    fed, fed_norm = (capi.BatchStager(u8_shape=(B, HW, HW), depth=2, photo=True) for _ in range(2))
    fed_norm.set_normalize(MEAN, STD, clamp=True)
    src = np.random.RandomState(1).randint(0, 256, size=B * HW * HW * 3, dtype=np.uint8)
    for st in (fed, fed_norm):  # the same bytes in every slot
        for _ in range(2):
            host, slot = st.acquire()
            host[:] = src
            st.submit(slot)
            st.wait(slot)
            st.release(slot)
    variants = {"augment_u8_photo presets": (fed, None, None, None), "augment_u8_photo params, mean / std, clamp": (fed_norm, None, params, blocks)}
    closers = [fed, fed_norm]
    if has_resident:
        small, _ = filled_dataset(capi, B, 1)
        large, _ = filled_dataset(capi, KERNEL_N, 1)
        rng = np.random.default_rng(4)  # another draw every launch, 32 of them in turn: 1.2 GB of samples, more than the Infinity Cache holds
        drawn = [rng.choice(KERNEL_N, size=B, replace=False).astype(np.int32) for _ in range(32)]
        for name, ds, idx in (("arange(256) of 256", small, [np.arange(B, dtype=np.int32)]), ("256 drawn from 10000", large, drawn)):
            plain = capi.BatchStager(u8_shape=(B, HW, HW), resident=ds, depth=2)
            norm = capi.BatchStager(u8_shape=(B, HW, HW), resident=ds, depth=2)
            norm.set_normalize(MEAN, STD, clamp=True)
            variants[f"augment_u8_resident {name}, presets"] = (plain, idx, None, None)
            variants[f"augment_u8_resident {name}, params, mean / std, clamp"] = (norm, idx, params, blocks)
            closers += [plain, norm]
        closers += [small, large]
    T.cuda.synchronize()

    def run(st, idx, mats, blk, launches):
        capi.kernel_timing(1)
        for i in range(launches):
            _, slot = st.acquire()
            if idx is not None:
                st.indices(slot)[:] = idx[(run.count + i) % len(idx)]
            if mats is not None:
                st.matrices(slot)[:] = mats
            if blk is not None:
                st.photo(slot)[:] = blk
            st.submit(slot)
            st.wait(slot)
            st.release(slot)
        run.count += launches
        T.cuda.synchronize()
        capi.kernel_timing(0)
        rep = capi.kernel_timing_report()
        assert len(rep) == 1, rep
        (key, (n, ms)), = rep.items()
        assert n == launches, rep
        return key.split("|")[0], ms * 1e3 / n

    run.count = 0
    for v in variants.values():
        run(*v, 5)
    us = {k: [] for k in variants}
    for _ in range(5):  # (the variants alternate: a drift of the box shows in all)
        for k, v in variants.items():
            name, t = run(*v, 20)
            assert k.split(" ")[0] == name, (k, name)
            us[k].append(t)
    for c in closers:
        c.close()
    print(json.dumps(dict(B=B, H=HW, W=HW, runs=us)))


def worker(variant, tree):
    sys.path.insert(0, tree)
    import torch as T

    from cnn_amd import capi, hostapi

    assert T.cuda.is_available(), "resident_bench.py measures on the device: no GPU, no numbers"
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == os.path.abspath(tree), capi.__file__
    if variant == "kernel":
        return kernel_worker(T, capi, hostapi)
    assert variant in LOOP_VARIANTS, variant
    rs = np.random.RandomState(1234)
    net = hostapi.HostAlexNet(3)
    net.set_params((rs.standard_normal(net.n_params) * 0.1).astype(np.float32))
    labels = (T.arange(B, device="cuda") % 3).to(T.int32)
    params = hostapi.augment_params(np.random.default_rng(2), B, HW, HW, HW, HW)
    blocks = hostapi.photo_params(np.random.default_rng(3), B, HW, HW)
    per_sample, closers = 200, []
    if variant == "unstaged":
        x = T.rand((B, 3, HW, HW), device="cuda")

        def loop(steps):
            for _ in range(steps):
                net.train_step(x, labels, 1e-3)
    elif variant in ("resident", "resident_depth3", "resident_gather_only"):
        ds, _ = filled_dataset(capi, LOOP_N, 1234)
        stager = capi.BatchStager(u8_shape=(B, HW, HW), resident=ds, depth=3 if variant == "resident_depth3" else 2)
        stager.set_normalize(MEAN, STD, clamp=True)
        closers = [stager, ds]
        per_epoch = LOOP_N // B
        order = np.concatenate([hostapi.epoch_order(LOOP_N, B, 7, e, drop_last=True) for e in range(-(-per_sample // per_epoch))])

        def loop(steps):
            if variant != "resident_gather_only":
                return net.train_epoch_resident(stager, order[:steps], 1e-3, params=lambda row: (params, blocks))
            net._resident_loop(stager, order[:steps], lambda row: (params, blocks), lambda *a: None)  # every gather, no step
    else:
        stager = capi.BatchStager(u8_shape=(B, HW, HW), depth=2, photo=True) if variant == "photo" else capi.BatchStager(u8_shape=(B, HW, HW), depth=2)
        if variant == "photo":
            stager.set_normalize(MEAN, STD, clamp=True)
        closers = [stager]
        for _ in range(2):  # synthetic images in both pinned slots (a real loader would decode into them)
            host, slot = stager.acquire()
            host[:] = rs.randint(0, 256, size=host.size, dtype=np.uint8)
            stager.submit(slot)

        def loop(steps):
            for _ in range(steps):
                _, slot = stager.acquire()
                if variant == "photo":
                    stager.matrices(slot)[:] = params
                    stager.photo(slot)[:] = blocks
                dev = stager.submit(slot)
                stager.wait(slot)
                net.train_step_ptr(dev, labels, B, HW, HW, 1e-3)
                stager.release(slot)

    loop(20)
    T.cuda.synchronize()
    rates = []
    for _ in range(4):
        t0 = time.perf_counter()
        loop(per_sample)
        T.cuda.synchronize()
        rates.append(B * per_sample / (time.perf_counter() - t0))
    for c in closers:
        c.close()
    net.close()
    print(json.dumps({"variant": variant, "tree": tree, "steps_per_sample": per_sample, "images_per_s": rates}))


def run_worker(variant, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--tree", tree]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:  # (a worker that failed ends the session: nothing more is started on the device)
        sys.exit(f"worker {variant} in {tree} failed with exit status {r.returncode}:\n{(r.stdout + r.stderr)[-3000:]}")
    print(f"  {variant} in {tree}: done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def tables(result):
    lines = []
    if "kernel" in result:
        lines += ["| kernel | us per launch: median (minimum - maximum) |", "|---|---|"]
        for name, v in result["kernel"]["us"].items():
            lines.append(f"| `{name}` | {v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f}) |")
    if "images_per_s" in result:
        lines += ["", "| variant | images/s: median (minimum - maximum) |", "|---|---|"]
        for name, v in result["images_per_s"].items():
            lines.append(f"| `{name}` | {v['median']:.0f} ({v['min']:.0f} - {v['max']:.0f}) |")
        lines.append(f"| requirement: `this:resident` above `this:photo`'s maximum | {'met' if result['resident_above_photo_max'] else 'NOT met'} |")
    return "\n".join(lines) + "\n"


def kernel_leg(parent, rounds):
    """the kernel worker in the parent's tree (if any) and in this one, alternating process by process; the runs of a tree are pooled"""
    trees = ([("parent", parent)] if parent else []) + [("this", ROOT)]
    runs = {}
    for _ in range(rounds):
        for t, tree in trees:
            for name, v in run_worker("kernel", tree)["runs"].items():
                runs.setdefault(f"{t}: {name}", []).extend(v)
    return dict(B=B, H=HW, W=HW, runs_per_variant=5 * rounds, us={k: spread(v) for k, v in runs.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-rounds", type=int, default=2)
    ap.add_argument("--legs", default="kernel,loop")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None, help="write the two tables (the body of profiles/resident_dataset.md) here")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, os.path.abspath(args.tree))
    legs = args.legs.split(",")
    assert set(legs) <= {"kernel", "loop"} and legs, args.legs
    parent = os.path.abspath(args.parent) if args.parent else None
    result = dict(batch=B)
    if "kernel" in legs:
        result["kernel"] = kernel_leg(parent, args.kernel_rounds)
    if "loop" in legs:
        result["samples_per_variant"] = 4 * args.rounds
        samples = {f"this:{v}": [] for v in LOOP_VARIANTS}
        for _ in range(args.rounds):
            for v in LOOP_VARIANTS:
                samples[f"this:{v}"] += run_worker(v, ROOT)["images_per_s"]
        result["images_per_s"] = {k: spread(v) for k, v in samples.items()}
        result["resident_above_photo_max"] = bool(result["images_per_s"]["this:resident"]["median"] > result["images_per_s"]["this:photo"]["max"])
    text = tables(result)
    print(text)
    for path, dump in ((args.out, lambda f: json.dump(result, f, indent=1)), (args.md, lambda f: f.write(text))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                dump(f)


if __name__ == "__main__":
    main()
