"""The cases and the record behind tests/golden/igemm_table.json: every row of kTiles (cnn_amd/csrc/conv_igemm.hip), forced with
CNN_AMD_IGEMM_CFG=<id>, one forward and one data-gradient call on each desc of DESCS.

tests/golden/make_igemm_table.py and tests/test_gpu_igemm_table.py call the SAME function here (the mechanism of tests/wgrad_sp_cases.py).
One record = one call: its launch log and the SHA-256 of its output, or the code it is refused with (a tile whose buffers exceed 160 KiB
of LDS on a desc).  The operands are the lattice operands of tests/exact.py, so every output also has one correct bit pattern: the
function compares each result with it and returns the differences -- the digests alone would pass a bug the recording library had.

The split tiles (Z > 1) are declined on planes this small at the card's CU count and leave the rule-based tile in the log; the record
holds that.  tests/test_gpu_igemm_tiles.py runs them at forced CU counts."""
import re

import numpy as np

from tests import exact as X
from tests import igemm_tiles as G
from tests.conv_route_cases import _Layer, _logged_outputs, _sha, key

DESCS = [
    (2, 6, 9, 10, 12, 3, 1, 1),    # Co = 12, Ci = 6: M <= 16 in both passes, so the 16-row tiles apply as well as the larger ones
    (3, 6, 10, 10, 40, 3, 1, 1),   # M = 40 forward (two 32-row blocks), M = 6 in the data gradient; rows of 10 floats with a ragged 16-byte tail;
                                   # tiles span images; whole-image staging
    # with 9 taps the filter slabs of the 128-row tiles with 16- and 32-channel chunks (224, 23) exceed the LDS on both descs above:
    # the first desc with 4 taps, on which every tile fits
    (2, 6, 9, 10, 12, 2, 1, 0),
]
CALLS = ("forward", "backward_data")


def options(cfg):
    """the TILE_OPTIONS of tests/test_gpu_scratch_contract.py"""
    return (("IGEMM_CFG", str(cfg)), ("CONV_ROWS", "0"), ("FWD_RD", "0"), ("DGRAD_RD", "0"))


def own_kernel(row, name):
    """is the launch-log name `name` the kernel of table row `row`, in any staging mode and either pass"""
    prefix = G.kernel_of(row)
    tail = r">/" if prefix.endswith(">") else r"(,img(\+mask(\+skip)?)?)?>/"
    return re.match(re.escape(prefix[:-1] if prefix.endswith(">") else prefix) + tail, name.split("|")[0]) is not None


class DeviceError(RuntimeError):
    """a HIP error: nothing more is started on the device"""


def table_record(T, repeats=1):
    """{"IGEMM_CFG=<id> / <desc key>": {call: {"log": ..., "sha": {...}} | {"log": ..., "rc": code}}}, the records whose digests did not
    repeat over `repeats` runs, and the differences from the integer truth (tests/exact.bits_differ reports)"""
    from contextlib import ExitStack

    from cnn_amd import capi

    rec, unstable, wrong = {}, [], []
    for cfg in sorted(G.source_table()):
        for desc in DESCS:
            where = f"IGEMM_CFG={cfg} / {key(desc)}"
            (x, w, b, dy), (y, _, _, dx) = X.lattice_conv(desc, X.seed_of(desc))
            with ExitStack() as stack:
                for name, value in options(cfg):
                    stack.enter_context(capi.option(name, value))
                # (under the options: they size the layer's workspace)
                L = _Layer(T, desc, 0, inputs=tuple(np.array(a) for a in (x, w, b, dy, np.maximum(x, np.float32(0)))))
                calls = {"forward": (lambda: {"y": L.conv.forward(L.x, L.w, L.b, L.y())}, y),
                         "backward_data": (lambda: {"dx": L.conv.backward_data(L.dy, L.w, L.dx())}, dx)}
                for call in CALLS:
                    fn, truth = calls[call]
                    first = None
                    for _ in range(repeats):
                        try:
                            out, log = _logged_outputs(T, fn)
                        except RuntimeError as e:
                            raise DeviceError(f"{where} {call}: {e}")
                        if isinstance(out, int):
                            if out >= 1000:
                                raise DeviceError(f"{where} {call}: HIP error {out}: {capi.load().cnn_amd_last_error().decode()}")
                            got = {"log": log, "rc": out}
                        else:
                            (o, t), = out.items()
                            got = {"log": log, "sha": {o: _sha(t)}}
                            report = X.bits_differ(t.detach().cpu().numpy(), truth, f"{where} {call}: {o}")
                            if report is not None and report not in wrong:
                                wrong.append(report)
                        if first is None:
                            first = got
                        assert got["log"] == first["log"] and got.get("rc") == first.get("rc"), (where, call, got, first)
                        if got.get("sha") != first.get("sha") and f"{where}:{call}" not in unstable:
                            unstable.append(f"{where}:{call}")
                    rec.setdefault(where, {})[call] = first
    return rec, unstable, wrong


def never_ran(rec):
    """the non-split ids whose own kernel is in none of their logs"""
    table, out = G.source_table(), []
    for cfg, row in sorted(table.items()):
        if row["Z"] > 1:
            continue
        logs = [name for desc in DESCS for r in rec[f"IGEMM_CFG={cfg} / {key(desc)}"].values() for name in r["log"]]
        if not any(own_kernel(row, name) for name in logs):
            out.append(cfg)
    return out
