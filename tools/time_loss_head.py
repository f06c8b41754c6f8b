#!/usr/bin/env python3
"""The loss head (linear_fwd+softmax_xent+dx+relu, 4608 -> 3, batch 256) per samples-per-workgroup setting and first_layer_finish:
alone, and inside the train step bench.py measures (the library's kernel timer sampling that one key in plain steps, every 4th launch).
The numbers of profiles/loss_head.md.

usage: python tools/time_loss_head.py [alone] [insitu] [S=1,2,4,8] [rounds=5]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cnn_amd import capi

HEAD, FINISH = "linear_fwd+softmax_xent+dx+relu", "first_layer_finish"
what = [a for a in sys.argv[1:] if "=" not in a] or ["alone", "insitu"]
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
ARMS = [int(s) for s in opts.get("S", "1,2,4,8").split(",")]
ROUNDS = int(opts.get("rounds", "5"))
B = 256


def sampled(fn, n, key, every=1):
    """us per launch of the kernels whose key contains `key` over n calls of fn"""
    capi.kernel_timing(2, key, every=every)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(0)
    cnt = sum(c for c, _ in rep.values())
    return sum(ms for _, ms in rep.values()) / cnt * 1e3 if cnt else float("nan")


def table(tag, rows):
    for name, v in rows.items():
        print(f"{tag:8s} {name:22s} " + " ".join(f"{t:6.2f}" for t in v) + f"   median {statistics.median(v):6.2f}  max-min {max(v) - min(v):5.2f} us")


def head_alone():
    g = torch.Generator(device="cuda").manual_seed(7)
    n_in = 4608
    x = torch.rand((B, n_in), generator=g, device="cuda") - 0.3
    w = torch.randn((n_in, 3), generator=g, device="cuda") * 0.05
    b = torch.randn((3,), generator=g, device="cuda") * 0.05
    labels = (torch.arange(B, device="cuda") % 3).to(torch.int32)
    logits, probs, delta = (torch.empty((B, 3), device="cuda") for _ in range(3))
    terms, dx = torch.empty((B,), device="cuda"), torch.empty((B, n_in), device="cuda")
    lib, P = capi.load(), capi._ptr

    def call():
        capi.check(lib.cnn_linear_forward_softmax_xent_dx(P(x), P(w), P(b), P(labels), P(logits), P(probs), P(delta), P(terms), P(dx), 1, B, n_in, 3,
                                                          capi._stream()), "cnn_linear_forward_softmax_xent_dx")

    for _ in range(300):
        call()
    rows = {f"head S={s}": [] for s in ARMS}
    for _ in range(ROUNDS):
        for s in ARMS:
            capi.set_option("HEAD_SAMPLES", s)
            rows[f"head S={s}"].append(sampled(call, 30, HEAD))
    capi.set_option("HEAD_SAMPLES", None)
    table("alone", rows)


def finish_alone():
    H = W = 224
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((B, 3, H, W), generator=g, device="cuda")
    w = torch.randn((16, 3, 3, 3), generator=g, device="cuda") * 0.1
    b = torch.randn((16,), generator=g, device="cuda") * 0.1
    conv = capi.Conv2d(B, 3, H, W, 16, 3, 2, 0)
    pf, pd = conv.prepared_buffers("cuda")
    pooled = torch.empty((B, 16, conv.Ho // 2, conv.Wo // 2), device="cuda")
    mask = torch.empty(pooled.shape, dtype=torch.int32, device="cuda")
    conv.relu_maxpool2_forward(x, w, b, pooled, mask)
    dpool = torch.rand(pooled.shape, generator=g, device="cuda") * 2 - 1
    gw, gb = torch.empty_like(w), torch.empty_like(b)

    def call():  # (lr = 0: the parameters stay what they are)
        conv.backward_weight_pooled2_sgd(x, dpool, mask, None, float(B), gw, gb, w, b, 0.0, 1.0, pf, pd)

    for _ in range(30):
        call()
    table("alone", {FINISH: [sampled(call, 30, FINISH) for _ in range(ROUNDS)]})


def in_situ():
    import bench

    run = bench.make_runner("alexnet", "layer", B, torch, capi, 1, 0, None)
    step = run["step"]

    def settle(n=20):
        for _ in range(n):
            step()
        run["flush"]()
        torch.cuda.synchronize()

    settle(300)
    rows = {f"head S={s}": [] for s in ARMS}
    fin = []
    for _ in range(ROUNDS):
        for s in ARMS:
            capi.set_option("HEAD_SAMPLES", s)
            settle()
            rows[f"head S={s}"].append(sampled(step, 100, HEAD, every=4))
        capi.set_option("HEAD_SAMPLES", None)
        settle()
        fin.append(sampled(step, 100, FINISH, every=4))
    run["flush"]()
    torch.cuda.synchronize()
    rows[FINISH] = fin
    table("in situ", rows)
    run["close"]()


if "alone" in what:
    head_alone()
    finish_alone()
if "insitu" in what:
    in_situ()
