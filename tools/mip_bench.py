#!/usr/bin/env python3
"""The numbers of the half-size levels in profiles/resident_dataset.md.  Needs an MI355X.  The method and the workers' building blocks are
tools/resident_bench.py's: fresh processes, the variants alternating, medians with minimum and maximum.
(A) the gather alone, B = 256, 224 x 224 output, 10 000 samples, another 256 indices every launch, on the library's per-launch HIP events:
      parent   augment_u8_resident in the parent's tree (--parent DIR: its own tools/resident_bench.py kernel worker), presets (one tap)
               and sampled maps (four taps)
      one      the same two in this tree out of a one-level dataset
      level0   augment_u8_resident_levels out of a two-level dataset of the same 224 x 224 samples: every map's scale is below 2, every
               sample sits on level 0, so the only difference to `one` is the kernel
      mixed    augment_u8_resident_levels out of a three-level dataset of 512 x 512 samples: a third of the batch a 224 x 224 crop at a half-pixel offset
               (level 0), a third the whole image (scale 2.29: level 1), a third at scale 4 (level 2; three quarters of those outputs lie outside
               the source and are fill)
    The processes of the two trees alternate; the runs of a variant are pooled.
(B) cnn_dataset_write of 10 000 images of 256 x 256 in blocks of 256 from pageable memory, one level against four: host clock around
    all the writes of a fresh dataset, alternating, fresh process each.
(C) the staged training loop of the reference net at B = 256 in images/s out of a one-level and a two-level dataset of 4096 samples
    (resident_bench.py's `resident` and `resident_depth3` loops; the maps stay below scale 2), alternating process by process.

usage: mip_bench.py [--parent DIR] [--rounds 2] [--legs kernel,write,loop] [--out FILE.json]
  (worker)  --worker NAME : one process, prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_bench as RB  # noqa: E402

B, HW = RB.B, RB.HW
WRITE_N, WRITE_HW = 10000, 256


def filled(capi, n, hw, levels, seed):
    block = np.random.RandomState(seed).randint(0, 256, size=(256, hw, hw, 3), dtype=np.uint8)
    ds = capi.ResidentDataset(n, hw, hw, levels=levels)
    for first in range(0, n, 256):
        count = min(256, n - first)
        ds.write(first, block[:count], (np.arange(first, first + count) % 3).astype(np.int32))
    return ds


def kernel_worker(T, capi, hostapi):
    params = hostapi.augment_params(np.random.default_rng(2), B, HW, HW, HW, HW)
    blocks = hostapi.photo_params(np.random.default_rng(3), B, HW, HW)
    assert all(capi.augment_level(m, 2)[0] == 0 for m in params), "the sampled maps stay below scale 2"
    rng = np.random.default_rng(4)
    drawn = [rng.choice(RB.KERNEL_N, size=B, replace=False).astype(np.int32) for _ in range(32)]
    mixed = np.empty((B, 6), np.float32)
    mixed[0::3] = [1, 0, 144.5, 0, 1, 144.5]
    mixed[1::3] = capi.augment_matrix([], 512, 512, HW, HW)
    mixed[2::3] = [4, 0, 1.5, 0, 4, 1.5]
    assert [capi.augment_level(m, 3)[0] for m in mixed[:3]] == [0, 1, 2]
    stores = {"one": filled(capi, RB.KERNEL_N, HW, 1, 1), "level0": filled(capi, RB.KERNEL_N, HW, 2, 1), "mixed": filled(capi, RB.KERNEL_N, 512, 3, 1)}
    variants, closers = {}, []
    for name, ds in stores.items():
        plain = capi.BatchStager(u8_shape=(B, HW, HW), resident=ds, depth=2)
        norm = capi.BatchStager(u8_shape=(B, HW, HW), resident=ds, depth=2)
        norm.set_normalize(RB.MEAN, RB.STD, clamp=True)
        closers += [plain, norm]
        if name == "mixed":
            variants["mixed: levels 0..2 of 512 x 512, mean / std, clamp"] = (norm, mixed, blocks)
        else:
            variants[f"{name}: presets"] = (plain, None, None)
            variants[f"{name}: params, mean / std, clamp"] = (norm, params, blocks)
    T.cuda.synchronize()
    count = [0]

    def run(st, mats, blk, launches):
        capi.kernel_timing(1)
        for i in range(launches):
            _, slot = st.acquire()
            st.indices(slot)[:] = drawn[(count[0] + i) % len(drawn)]
            if mats is not None:
                st.matrices(slot)[:] = mats
                st.photo(slot)[:] = blk
            st.submit(slot)
            st.wait(slot)
            st.release(slot)
        count[0] += launches
        T.cuda.synchronize()
        capi.kernel_timing(0)
        rep = capi.kernel_timing_report()
        assert len(rep) == 1, rep
        (key, (n, ms)), = rep.items()
        assert n == launches, rep
        return key.split("|")[0], ms * 1e3 / n

    for v in variants.values():
        run(*v, 5)
    us = {k: [] for k in variants}
    for _ in range(5):
        for k, v in variants.items():
            name, t = run(*v, 20)
            assert name == ("augment_u8_resident" if k.startswith("one") else "augment_u8_resident_levels"), (k, name)
            us[k].append(t)
    for c in closers + list(stores.values()):
        c.close()
    print(json.dumps(dict(runs=us)))


def write_worker(T, capi, levels):
    block = np.random.RandomState(5).randint(0, 256, size=(256, WRITE_HW, WRITE_HW, 3), dtype=np.uint8)
    warm = capi.ResidentDataset(256, WRITE_HW, WRITE_HW, levels=levels)
    warm.write(0, block)
    warm.close()
    seconds = []
    for _ in range(3):
        ds = capi.ResidentDataset(WRITE_N, WRITE_HW, WRITE_HW, levels=levels)
        T.cuda.synchronize()
        t0 = time.perf_counter()
        for first in range(0, WRITE_N, 256):
            ds.write(first, block[:min(256, WRITE_N - first)])
        seconds.append(time.perf_counter() - t0)
        ds.close()
    print(json.dumps(dict(levels=levels, us_per_image=[s * 1e6 / WRITE_N for s in seconds])))


def loop_worker(T, capi, hostapi, levels, depth):
    rs = np.random.RandomState(1234)
    net = hostapi.HostAlexNet(3)
    net.set_params((rs.standard_normal(net.n_params) * 0.1).astype(np.float32))
    params = hostapi.augment_params(np.random.default_rng(2), B, HW, HW, HW, HW)
    blocks = hostapi.photo_params(np.random.default_rng(3), B, HW, HW)
    ds = filled(capi, RB.LOOP_N, HW, levels, 1234)
    stager = capi.BatchStager(u8_shape=(B, HW, HW), resident=ds, depth=depth)
    stager.set_normalize(RB.MEAN, RB.STD, clamp=True)
    per_sample, per_epoch = 200, RB.LOOP_N // B
    order = np.concatenate([hostapi.epoch_order(RB.LOOP_N, B, 7, e, drop_last=True) for e in range(-(-per_sample // per_epoch))])
    loop = lambda steps: net.train_epoch_resident(stager, order[:steps], 1e-3, params=lambda row: (params, blocks))
    loop(20)
    T.cuda.synchronize()
    rates = []
    for _ in range(4):
        t0 = time.perf_counter()
        loop(per_sample)
        T.cuda.synchronize()
        rates.append(B * per_sample / (time.perf_counter() - t0))
    stager.close()
    ds.close()
    net.close()
    print(json.dumps(dict(images_per_s=rates)))


def worker(name):
    sys.path.insert(0, ROOT)
    import torch as T

    from cnn_amd import capi, hostapi

    assert T.cuda.is_available(), "mip_bench.py measures on the device: no GPU, no numbers"
    if name == "kernel":
        return kernel_worker(T, capi, hostapi)
    kind, levels, *rest = name.split(":")
    if kind == "write":
        return write_worker(T, capi, int(levels))
    return loop_worker(T, capi, hostapi, int(levels), int(rest[0]))


def run_worker(cmd):
    r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=400)
    if r.returncode != 0:  # (a worker that failed ends the session: nothing more is started on the device)
        sys.exit(f"worker {cmd} failed with exit status {r.returncode}:\n{(r.stdout + r.stderr)[-3000:]}")
    print(f"  {' '.join(cmd[-3:])}: done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--legs", default="kernel,write,loop")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    me = os.path.abspath(__file__)
    legs, result = args.legs.split(","), {}
    if "kernel" in legs:
        runs = {}
        for _ in range(args.rounds):
            if args.parent:
                parent = os.path.abspath(args.parent)
                got = run_worker([os.path.join(parent, "tools", "resident_bench.py"), "--worker", "kernel", "--tree", parent])["runs"]
                for k, v in got.items():
                    if k.startswith("augment_u8_resident 256 drawn"):
                        runs.setdefault("parent: " + k.split(", ", 1)[1], []).extend(v)
            for k, v in run_worker([me, "--worker", "kernel"])["runs"].items():
                runs.setdefault(k, []).extend(v)
        result["kernel_us"] = {k: RB.spread(v) for k, v in runs.items()}
    if "write" in legs:
        runs = {}
        for _ in range(args.rounds):
            for levels in (1, 4):
                runs.setdefault(f"levels={levels}", []).extend(run_worker([me, "--worker", f"write:{levels}"])["us_per_image"])
        result["write_us_per_image"] = {k: RB.spread(v) for k, v in runs.items()}
    if "loop" in legs:
        runs = {}
        for _ in range(args.rounds):
            for depth in (2, 3):
                for levels in (1, 2):
                    runs.setdefault(f"levels={levels} depth={depth}", []).extend(run_worker([me, "--worker", f"loop:{levels}:{depth}"])["images_per_s"])
        result["loop_images_per_s"] = {k: RB.spread(v) for k, v in runs.items()}
    for leg, table in result.items():
        print(f"| {leg} | median (minimum - maximum) |\n|---|---|")
        for k, v in table.items():
            print(f"| `{k}` | {v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f}) |")
        print()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
