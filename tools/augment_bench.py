#!/usr/bin/env python3
"""The numbers of profiles/augmentation.md: what augmentation on the device costs.  Needs an MI355X.
(A) the kernel: one cnn_augment_u8 launch (augment_u8) at B = 256, 224 x 224 -> 224 x 224 against the yardstick u8hwc_to_f32chw (the
    plain u8 stager's conversion: the same stores, a quarter of the reads) on the same bytes, with identity matrices and with
    hostapi.augment_params matrices.  Both kernels run where they run in use, on a stager's copy stream behind its upload, so the clock
    is the library's own per-launch HIP events (cnn_amd_kernel_timing_enable) around each launch.  ONE process, the three variants
    alternating run by run, five runs each; a run is the mean over 20 launches.  Beside them the byte floor: 154 MB written and 38.5 MB
    read at the HBM rate a float4 copy reaches.  The photo leg: the same launch with the photometric epilogue (augment_u8_photo, the
    photo stager's kernel) -- with the block acquire() presets, and with hostapi.photo_params blocks, ImageNet's mean / std and the clamp
    beside the sampled matrices -- in the same alternation.  With --parent the worker also runs in the parent's tree (its geometric
    variants only), the two trees alternating process by process, --kernel-rounds times: the parent's geometric launch is the yardstick
    of the epilogue, and this tree's geometric launch must not have moved.
(B) the staged-input training loop of the reference net at B = 256 in images/s (bench.py --staged-input's u8 leg: acquire, submit, wait,
    train step, release), every variant a fresh process, the variants alternating round by round:
      u8            the plain u8 stager; run with --parent in the parent's tree and libraries, and in this tree
      aug_identity  the augmenting stager with the matrices acquire() presets
      aug_params    the same with a batch of augment_params matrices copied into the slot every step (sampled ahead of the loop: a
                    loader thread's work)
      photo_params  the photo stager with augment_params matrices and photo_params blocks copied into the slot every step, ImageNet's
                    mean / std and the clamp
    A sample is a host clock around a loop of steps that ends in a synchronise.  The expectation: aug_* no slower than the parent's median
    minus the parent's own maximum - minimum.

usage: augment_bench.py [--parent DIR] [--rounds 5] [--kernel-rounds 3] [--legs kernel,loop] [--out FILE.json] [--md FILE.md]
  --parent DIR : a checkout of the PARENT commit with its libraries built (cnn_amd/lib/*.so); without it only this tree is measured
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
HBM_BYTES_PER_S = 6.29e12  # a float4 copy on this chip (8.0 TB/s on paper)


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def kernel_worker(T, capi, hostapi):
    rs = np.random.RandomState(1)
    src = rs.randint(0, 256, size=B * HW * HW * 3, dtype=np.uint8)
    params = hostapi.augment_params(np.random.default_rng(2), B, HW, HW, HW, HW)
    plain = capi.BatchStager(u8_shape=(B, HW, HW), depth=2)
    aug = capi.BatchStager(u8_shape=(B, HW, HW), depth=2, augment=True)
    stagers = [plain, aug]
    has_photo = hasattr(hostapi, "photo_params")  # (the parent's tree has no photo stager)
    if has_photo:
        blocks = hostapi.photo_params(np.random.default_rng(3), B, HW, HW)
        photo, photo_norm = (capi.BatchStager(u8_shape=(B, HW, HW), depth=2, photo=True) for _ in range(2))
        photo_norm.set_normalize(MEAN, STD, clamp=True)
        stagers += [photo, photo_norm]
    for st in stagers:  # the same bytes in every slot
        for _ in range(2):
            host, slot = st.acquire()
            host[:] = src
            st.submit(slot)
            st.wait(slot)
            st.release(slot)
    T.cuda.synchronize()

    def run(st, mats, launches, blocks=None):
        capi.kernel_timing(1)
        for _ in range(launches):
            _, slot = st.acquire()
            if mats is not None:
                st.matrices(slot)[:] = mats
            if blocks is not None:
                st.photo(slot)[:] = blocks
            st.submit(slot)
            st.wait(slot)
            st.release(slot)
        T.cuda.synchronize()
        capi.kernel_timing(0)
        rep = capi.kernel_timing_report()
        assert len(rep) == 1, rep
        (key, (n, ms)), = rep.items()
        assert n == launches, rep
        return key.split("|")[0], ms * 1e3 / n

    variants = {"u8hwc_to_f32chw": (plain, None), "augment_u8 identity": (aug, None), "augment_u8 augment_params": (aug, params)}
    if has_photo:
        variants.update({"augment_u8_photo identity, preset blocks": (photo, None), "augment_u8_photo augment_params, preset blocks": (photo, params),
                         "augment_u8_photo augment_params, photo_params blocks, mean / std, clamp": (photo_norm, params, blocks)})
    for st, *rest in variants.values():
        run(st, rest[0], 5, *rest[1:])
    us = {k: [] for k in variants}
    for _ in range(5):  # (the variants alternate: a drift of the box shows in all)
        for k, (st, *rest) in variants.items():
            name, t = run(st, rest[0], 20, *rest[1:])
            assert k.split(" ")[0] == name, (k, name)
            us[k].append(t)
    for st in stagers:
        st.close()
    written, read = B * 3 * HW * HW * 4, B * HW * HW * 3
    print(json.dumps(dict(B=B, H=HW, W=HW, runs=us, us={k: spread(v) for k, v in us.items()}, bytes_written=written, bytes_read=read,
                          floor_us=(written + read) / HBM_BYTES_PER_S * 1e6)))


def worker(variant, tree):
    sys.path.insert(0, tree)
    import torch as T

    from cnn_amd import capi, hostapi

    assert T.cuda.is_available(), "augment_bench.py measures on the device: no GPU, no numbers"
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == os.path.abspath(tree), capi.__file__
    if variant == "kernel":
        return kernel_worker(T, capi, hostapi)
    assert variant in ("u8", "aug_identity", "aug_params", "photo_params"), variant
    rs = np.random.RandomState(1234)
    net = hostapi.HostAlexNet(3)
    net.set_params((rs.standard_normal(net.n_params) * 0.1).astype(np.float32))
    labels = (T.arange(B, device="cuda") % 3).to(T.int32)
    if variant == "photo_params":
        stager = capi.BatchStager(u8_shape=(B, HW, HW), depth=2, photo=True)
        stager.set_normalize(MEAN, STD, clamp=True)
    else:
        stager = capi.BatchStager(u8_shape=(B, HW, HW), depth=2) if variant == "u8" else capi.BatchStager(u8_shape=(B, HW, HW), depth=2, augment=True)
    params = hostapi.augment_params(np.random.default_rng(2), B, HW, HW, HW, HW) if variant in ("aug_params", "photo_params") else None
    blocks = hostapi.photo_params(np.random.default_rng(3), B, HW, HW) if variant == "photo_params" else None
    for _ in range(2):  # synthetic images in both pinned slots (a real loader would decode into them)
        host, slot = stager.acquire()
        host[:] = rs.randint(0, 256, size=host.size, dtype=np.uint8)
        stager.submit(slot)

    def step():
        _, slot = stager.acquire()
        if params is not None:
            stager.matrices(slot)[:] = params
        if blocks is not None:
            stager.photo(slot)[:] = blocks
        dev = stager.submit(slot)
        stager.wait(slot)
        net.train_step_ptr(dev, labels, B, HW, HW, 1e-3)
        stager.release(slot)

    per_sample = 200
    for _ in range(20):
        step()
    T.cuda.synchronize()
    rates = []
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(per_sample):
            step()
        T.cuda.synchronize()
        rates.append(B * per_sample / (time.perf_counter() - t0))
    stager.close()
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
        k = result["kernel"]
        lines += ["| kernel | us per launch: median (minimum - maximum) |", "|---|---|"]
        for name, v in k["us"].items():
            lines.append(f"| `{name}` | {v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f}) |")
        lines.append(f"| byte floor: {k['bytes_written'] / 1e6:.1f} MB written + {k['bytes_read'] / 1e6:.1f} MB read at {HBM_BYTES_PER_S / 1e12:.2f} TB/s | {k['floor_us']:.1f} |")
    if "images_per_s" in result:
        lines += ["", "| variant | images/s: median (minimum - maximum) |", "|---|---|"]
        for name, v in result["images_per_s"].items():
            lines.append(f"| `{name}` | {v['median']:.0f} ({v['min']:.0f} - {v['max']:.0f}) |")
        if "bar_images_per_s" in result:
            lines.append(f"| bar: the parent's median minus its own maximum - minimum | {result['bar_images_per_s']:.0f} |")
    return "\n".join(lines) + "\n"


def kernel_leg(parent, rounds):
    """the kernel worker in the parent's tree (if any) and in this one, alternating process by process; the runs of a tree are pooled"""
    trees = ([("parent", parent)] if parent else []) + [("this", ROOT)]
    runs, last = {}, None
    for _ in range(rounds):
        for t, tree in trees:
            last = run_worker("kernel", tree)
            for name, v in last["runs"].items():
                runs.setdefault(f"{t}: {name}" if parent else name, []).extend(v)
    return dict(B=last["B"], H=last["H"], W=last["W"], runs_per_variant=5 * rounds, us={k: spread(v) for k, v in runs.items()},
                bytes_written=last["bytes_written"], bytes_read=last["bytes_read"], floor_us=last["floor_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-rounds", type=int, default=3)
    ap.add_argument("--legs", default="kernel,loop")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None, help="write the two tables (the body of profiles/augmentation.md) here")
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
        plan = ([("parent", parent, "u8")] if parent else []) + [("this", ROOT, v) for v in ("u8", "aug_identity", "aug_params", "photo_params")]
        result["samples_per_variant"] = 4 * args.rounds
        samples = {f"{t}:{v}": [] for t, _, v in plan}
        for _ in range(args.rounds):
            for t, tree, v in plan:
                samples[f"{t}:{v}"] += run_worker(v, tree)["images_per_s"]
        result["images_per_s"] = {k: spread(v) for k, v in samples.items()}
    if parent and "loop" in legs:
        p = result["images_per_s"]["parent:u8"]
        result["bar_images_per_s"] = p["median"] - (p["max"] - p["min"])
        result["within_bar"] = {k: bool(v["median"] >= result["bar_images_per_s"]) for k, v in result["images_per_s"].items()
                                if k.startswith("this:aug") or k.startswith("this:photo")}
    text = tables(result)
    print(text)
    for path, dump in ((args.out, lambda f: json.dump(result, f, indent=1)), (args.md, lambda f: f.write(text))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                dump(f)


if __name__ == "__main__":
    main()
