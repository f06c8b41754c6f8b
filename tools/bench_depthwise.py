#!/usr/bin/env python3
"""The numbers of profiles/depthwise.md: the three depthwise passes (CNN_CONV2D_DEPTHWISE, conv_depthwise.hip) on the depthwise layers
of MobileNet-V1 at B = 64 (all 3x3, pad 1), timed with the library's kernel timer (HIP events around every launch) in ONE
process.  Per shape and pass:
  (a) the time: the median over REGIONS regions of REPS calls each, after a warm-up, of the sum of the kernels the call launches (the
      weight gradient: dw_wgrad + slab_reduce);
  (b) the algorithmic bytes -- forward x + y, data gradient dy + dx, weight gradient x + dy -- over that time, as a share of the
      6.3 TB/s an MI355X streams from HBM (tensors of less than 256 MiB in total can stay in the Infinity Cache between calls);
  (c) cnn_relu_forward over as many elements as the layer's x (it moves the bytes of a stride-1 forward), alternating with the passes;
  (d) the dense route on expand_filters(w) -- what a caller without the flag has to run -- for the same shape, alternating too.
Then one train step of HostSequential(stacks.mobilenet_v1()) at B = 64: HIP events around back-to-back steps, and the kernel timer's
breakdown of one region.  Needs an MI355X: no device, no numbers.

usage: bench_depthwise.py [--out profiles/depthwise.md] [--json FILE] [--regions 7] [--reps 20] [--no-step]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 64
SHAPES = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2), (512, 14, 1), (512, 14, 2), (1024, 7, 1)]  # (C, H = W, stride)
HBM_TBS = 6.3


def kernel_us(T, capi, fn, reps):
    """us per call of fn, summed over the kernels it launches, and their names"""
    T.cuda.synchronize()
    capi.kernel_timing(1)
    try:
        for _ in range(reps):
            fn()
        T.cuda.synchronize()
        rep = capi.kernel_timing_report()
    finally:
        capi.kernel_timing(0)
    return sum(ms for _, ms in rep.values()) * 1e3 / reps, sorted(k.split("|")[0] for k in rep)


def expand_filters(w):
    Cn, _, k, _ = w.shape
    out = np.zeros((Cn, Cn, k, k), w.dtype)
    idx = np.arange(Cn)
    out[idx, idx] = w[:, 0]
    return out


def layer_numbers(T, capi, Cn, H, s, regions, reps):
    lib = capi.load()
    rs = np.random.RandomState(Cn + H + s)
    Ho = capi.conv_out_dim(H, 3, s, 1)
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    x, dy = dev(rs.standard_normal((B, Cn, H, H))), dev(rs.standard_normal((B, Cn, Ho, Ho)))
    w_host = (rs.standard_normal((Cn, 1, 3, 3)) / 3).astype(np.float32)
    w, bias, W = dev(w_host), dev(rs.standard_normal(Cn) * 0.1), dev(expand_filters(w_host))
    y, dx, relu_out = T.empty_like(dy), T.empty_like(x), T.empty_like(x)
    gw, gb, GW = T.empty_like(w), T.empty_like(bias), T.empty_like(W)
    d = capi.ConvDesc(B, Cn, H, H, Cn, 3, s, 1, capi.DEPTHWISE)
    ws_bytes = int(lib.cnn_conv2d_workspace_bytes(C.byref(d)))
    ws = T.empty(ws_bytes, dtype=T.uint8, device="cuda")
    dense = capi.Conv2d(B, Cn, H, H, Cn, 3, s, 1)
    p, st = capi._ptr, capi._stream

    def dw(call, *args):
        return lambda: capi.check(getattr(lib, call)(C.byref(d), *args, p(ws), ws_bytes, st()), call)

    fns = {
        "fwd": dw("cnn_conv2d_forward", p(x), p(w), p(bias), p(y)),
        "dgrad": dw("cnn_conv2d_backward_data", p(dy), p(w), p(dx)),
        "wgrad": dw("cnn_conv2d_backward_weight", p(x), p(dy), p(gw), p(gb), float(B)),
        "relu": lambda: capi.relu_forward(x, relu_out),
        "dense fwd": lambda: dense.forward(x, W, bias, y),
        "dense dgrad": lambda: dense.backward_data(dy, W, dx),
        "dense wgrad": lambda: dense.backward_weight(x, dy, float(B), GW, gb),
    }
    names = {}
    for k, fn in fns.items():  # warm-up (code objects, attributes)
        _, names[k] = kernel_us(T, capi, fn, 3)
    us = {k: [] for k in fns}
    for _ in range(regions):  # (everything alternates region by region: a drift of the machine shows in all of them)
        for k, fn in fns.items():
            us[k].append(kernel_us(T, capi, fn, reps)[0])
    nx, ny = B * Cn * H * H, B * Cn * Ho * Ho
    return dict(C=Cn, H=H, s=s, bytes={"fwd": 4 * (nx + ny), "dgrad": 4 * (nx + ny), "wgrad": 4 * (nx + ny), "relu": 8 * nx},
                us={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in us.items()}, kernels=names)


def step_numbers(T, capi, regions):
    from cnn_amd import hostapi, stacks

    net = hostapi.HostSequential(stacks.mobilenet_v1())
    net.set_params(stacks.he_init(net.layout, 11))
    x = T.from_numpy(np.random.RandomState(3).rand(B, 3, 224, 224).astype(np.float32)).cuda()
    labels = T.from_numpy((np.arange(B) % 3).astype(np.int32)).cuda()
    step = lambda: net.train_step(x, labels, 1e-3)  # noqa: E731
    for _ in range(5):
        step()
    T.cuda.synchronize()
    ms = []
    for _ in range(regions):
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / 10)
    T.cuda.synchronize()
    capi.kernel_timing(1)
    try:
        for _ in range(5):
            step()
        net.flush()
        T.cuda.synchronize()
        rep = capi.kernel_timing_report()
    finally:
        capi.kernel_timing(0)
    by_kernel = {}
    for key, (cnt, tot) in rep.items():
        name = key.split("|")[0].split("<")[0]
        c0, t0 = by_kernel.get(name, (0, 0.0))
        by_kernel[name] = (c0 + cnt / 5, t0 + tot / 5)
    net.close()
    return dict(ms=dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms))), n_params=int(net.n_params),
                kernels=sorted(((k, c, t) for k, (c, t) in by_kernel.items()), key=lambda r: -r[2]))


def markdown(layers, step, regions, reps):
    out = ["# Depthwise convolution: the three passes on MobileNet-V1's depthwise layers", "",
           f"Written by `tools/bench_depthwise.py` on an MI355X.  B = {B}, 3x3, pad 1.  Times are the library's kernel timer (HIP events around",
           f"every launch), the median (minimum - maximum) over {regions} regions of {reps} calls, one process, every row's calls alternating",
           "region by region.  Bytes are algorithmic (forward x + y, data gradient dy + dx, weight gradient x + dy); the share is of the",
           f"{HBM_TBS} TB/s an MI355X streams from HBM.  `relu` is `cnn_relu_forward` over the layer's x: the volume of a stride-1 forward.",
           "`dense` is the same shape through the dense route on block-diagonal filters `[C][C][3][3]`.", "",
           "| layer | pass | us | TB/s | share of 6.3 TB/s | relu us | pass / relu (per byte) | dense us | dense / depthwise |",
           "|---|---|---|---|---|---|---|---|---|"]
    for L in layers:
        mb = (L["bytes"]["fwd"]) / 2 ** 20
        note = " (fits the Infinity Cache)" if mb < 256 else ""
        for k in ("fwd", "dgrad", "wgrad"):
            u, r, dn = L["us"][k], L["us"]["relu"], L["us"]["dense " + k]
            tbs = L["bytes"][k] / u["median"] * 1e-6
            per_byte = (u["median"] / L["bytes"][k]) / (r["median"] / L["bytes"]["relu"])
            out.append(f"| {L['C']}@{L['H']} s{L['s']}, {mb:.0f} MiB{note} | {k} | {u['median']:.1f} ({u['min']:.1f} - {u['max']:.1f}) | {tbs:.2f} | "
                       f"{100 * tbs / HBM_TBS:.0f} % | {r['median']:.1f} | {per_byte:.2f} | {dn['median']:.1f} | {dn['median'] / u['median']:.1f}x |")
    out += ["", "Kernels per call: " + "; ".join(f"{L['C']}@{L['H']} s{L['s']}: " + ", ".join(f"{k} = {' + '.join(v)}" for k, v in L["kernels"].items()
                                                                                                if not k.startswith("relu")) for L in layers[:2]), ""]
    slower = [f"{L['C']}@{L['H']} s{L['s']} {k}" for L in layers for k in ("fwd", "dgrad", "wgrad") if L["us"]["dense " + k]["median"] <= L["us"][k]["median"]]
    out += ["Depthwise faster than the dense route on every shape and pass: " + ("yes" if not slower else "NO -- " + ", ".join(slower)), ""]
    if step:
        out += [f"## One train step of `HostSequential(stacks.mobilenet_v1())`, B = {B}", "",
                f"{step['ms']['median']:.2f} ms per step (minimum {step['ms']['min']:.2f}, maximum {step['ms']['max']:.2f}; {regions} regions of 10 back-to-back steps, HIP",
                f"events), {step['n_params']} parameters.  No threshold applies.  Kernel timer, per step (a run of its own: the timer serialises the streams):", "",
                "| kernel | launches | ms |", "|---|---|---|"]
        out += [f"| `{k}` | {c:.0f} | {t:.3f} |" for k, c, t in step["kernels"][:24]]
        out += [f"| (sum of all {len(step['kernels'])}) | {sum(c for _, c, _ in step['kernels']):.0f} | {sum(t for _, _, t in step['kernels']):.3f} |", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthwise.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import torch as T

    from cnn_amd import capi

    assert T.cuda.is_available(), "bench_depthwise.py measures on the device: no GPU, no numbers"
    layers = []
    for Cn, H, s in SHAPES:
        layers.append(layer_numbers(T, capi, Cn, H, s, args.regions, args.reps))
        print(f"{Cn}@{H} s{s}: " + ", ".join(f"{k} {v['median']:.1f} us" for k, v in layers[-1]["us"].items()), flush=True)
        T.cuda.empty_cache()
    step = None if args.no_step else step_numbers(T, capi, args.regions)
    text = markdown(layers, step, args.regions, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")
    if args.json:
        json.dump(dict(layers=layers, step=step), open(args.json, "w"), indent=1)
    print(text)


if __name__ == "__main__":
    main()
