#!/usr/bin/env python3
"""Records the optimizer state files of tests/test_gpu_optstate_files.py: tests/golden/optstate_{sgd,adam,lamb,lars}.state and
optstate_kat.json.  Needs the GPU and built libraries.

On the small_bn net of tests/test_gpu_optimizer.py (3x32x32 input, batch 4: 4563 parameters, so the four files together are about
110 KB) with a fixed seed it takes two train_steps under each of the four optimizers, with non-default options that include
decay_bias_and_norm, adapt_bias_and_norm and decoupled, and saves the state.  The JSON carries n_params, the options, the step
counter and the commit whose libraries wrote the files.

The files pin the four on-disk formats against the code that shipped them: they were recorded ONCE, with the libraries of the commit
named in the JSON (the last one before the host optimizer code became one mechanism), and are not re-recorded when the writer
changes -- a writer that no longer reproduces them byte for byte has changed the format.
usage: python tests/golden/make_optstate_kat.py --commit HASH [--out DIR]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import torch

from tests.test_gpu_optimizer import make_net, net_inputs

SEED, STEPS, LR = 700, 2, 1e-2
KAT = {
    "sgd": dict(setter="set_optimizer", magic="CNNAOPT1", header_bytes=32, arenas=1, first_option_at=16,
                options=dict(momentum=0.85, weight_decay=1.5e-3, nesterov=True, decay_bias_and_norm=True)),
    "adam": dict(setter="set_adam", magic="CNNAADM1", header_bytes=48, arenas=2, first_option_at=24,
                 options=dict(beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=3e-3, decoupled=True, decay_bias_and_norm=True)),
    "lamb": dict(setter="set_lamb", magic="CNNALMB1", header_bytes=48, arenas=2, first_option_at=24,
                 options=dict(beta1=0.85, beta2=0.98, eps=1e-5, weight_decay=2e-2, decay_bias_and_norm=True, adapt_bias_and_norm=True)),
    "lars": dict(setter="set_lars", magic="CNNALRS1", header_bytes=48, arenas=1, first_option_at=16,
                 options=dict(momentum=0.7, weight_decay=1e-3, trust_coefficient=2e-3, eps=1e-7, nesterov=True, decay_bias_and_norm=False,
                              adapt_bias_and_norm=True)),
}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the libraries in use were built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    layout, p0, x, labels = net_inputs(torch, "small_bn", SEED)
    report = {"commit": args.commit, "net": "small_bn", "seed": SEED, "steps": STEPS, "lr": LR, "files": {}}
    for name, kat in KAT.items():
        net = make_net("small_bn")
        net.set_params(p0)
        getattr(net, kat["setter"])(**kat["options"])
        for _ in range(STEPS):
            net.train_step(x, labels, LR)
        path = os.path.join(args.out, f"optstate_{name}.state")
        net.save_optimizer_state(path)
        assert os.path.getsize(path) == kat["header_bytes"] + kat["arenas"] * 4 * net.n_params
        report["n_params"] = net.n_params
        report["files"][name] = dict(kat, file=os.path.basename(path), step=STEPS if name in ("adam", "lamb") else None)
        net.close()
    json.dump(report, open(os.path.join(args.out, "optstate_kat.json"), "w"), indent=1, sort_keys=True)
    print(f"{len(KAT)} state files, n_params = {report['n_params']} -> {args.out}")
