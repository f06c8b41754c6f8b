"""The cases and the record behind tests/golden/wgrad_sp_family.json: every instance and every epilogue path of the LDS-staged
output-stationary weight gradients (conv_wgrad_sp.hip, conv_wgrad_sp2.hip, conv_wgrad_sp_any.hip; shared pieces in wgrad_sp_common.h).

tests/golden/make_wgrad_sp_family.py and tests/test_gpu_wgrad_sp_family.py call the SAME function here (the mechanism of
tests/conv_route_cases.py, whose _Layer / _logged / _sha are reused).  One record = one backward_weight call: its launch log and the
SHA-256 of gw and gb.  Each case runs under the default stage partition and with SP_BLOCKS = 1 and 3: a pinned workgroup count makes
those two records independent of the device's CU count, and 3 gives several stages per workgroup with a ragged last one."""
from tests.conv_route_cases import _Layer, _logged, key

# (kernel name in the launch log, options, [(B, Ci, H, W, Co, k, s, pad)]): the smallest cases of tests/test_gpu_parity.py that reach
# every instance
SP = [
    (3, 64, 7, 7, 128, 3, 1, 1),     # sample pairs, odd batch
    (5, 40, 7, 7, 70, 3, 1, 1),      # ... partial tiles
    (1, 24, 14, 14, 100, 3, 1, 1),
    (1, 20, 28, 28, 72, 3, 1, 1),
    (1, 12, 56, 56, 40, 3, 1, 1),
    (2, 64, 3, 56, 64, 3, 1, 1),     # a halo row outside the image in every stage
    (1, 40, 6, 112, 100, 3, 1, 1),   # CT = 32: two waves per tile, partial both ways
    (1, 24, 9, 112, 70, 3, 1, 0),    # CT = 32, pad 0
]
SP2 = [
    (1, 40, 56, 56, 72, 3, 2, 1),    # CT = 32
    (3, 24, 28, 28, 100, 3, 2, 1),
    (5, 72, 14, 14, 40, 3, 2, 1),    # ragged row slots
    (2, 32, 27, 27, 64, 3, 2, 0),
    (3, 64, 13, 13, 128, 3, 2, 0),
]
SPA = [
    (2, 64, 9, 23, 64, 3, 1, 0),     # 21-column block
    (2, 40, 30, 50, 72, 3, 1, 1),    # 28-column block, partial tiles
    (1, 32, 6, 223, 40, 3, 1, 1),    # fix-ups on x and dy
    (2, 32, 32, 32, 32, 3, 1, 0),    # last block cut inside a unit
]
GROUPS = [
    ("wgrad_sp<", {"WGRAD_SP": "1"}, SP),
    ("wgrad_sp<", {"WGRAD_SP": "1", "SP_UNIT": "1"}, SP),  # the 4-byte DMA instances
    ("wgrad_sp2<", {"WGRAD_SP2": "2"}, SP2),
    ("wgrad_sp_any<", {"WGRAD_SP_ANY": "2"}, SPA),
]
PARTITIONS = [None, "1", "3"]  # SP_BLOCKS


def family_record(T, repeats=1):
    """{"<options> SP_BLOCKS=<n>|default / <desc key>": {"kernel": name prefix, "log": ..., "sha": {"gb", "gw"}}}; repeats > 1 (the
    maker): every call runs that often -- returns (record, [records whose digests did not repeat])"""
    from contextlib import ExitStack

    from cnn_amd import capi

    rec, unstable = {}, []
    for g, (kernel, options, cases) in enumerate(GROUPS):
        for i, case in enumerate(cases):
            for blocks in PARTITIONS:
                opts = dict(options, **({"SP_BLOCKS": blocks} if blocks else {}))
                where = " ".join(f"{k}={v}" for k, v in sorted(opts.items())) + " / " + key(case)
                with ExitStack() as stack:
                    for name, value in opts.items():
                        stack.enter_context(capi.option(name, value))
                    L = _Layer(T, case, 7000 + 100 * g + 10 * i)  # (under the options: they size the layer's workspace)

                    def backward_weight():
                        gw, gb = L.conv.backward_weight(L.x, L.dy, float(case[0]))
                        return {"gw": gw, "gb": gb}

                    got = [_logged(T, backward_weight) for _ in range(repeats)]
                assert all(r["log"] == got[0]["log"] and "sha" in r for r in got), (where, got)
                if any(r["sha"] != got[0]["sha"] for r in got):
                    unstable.append(where)
                rec[where] = dict(got[0], kernel=kernel)
    return rec, unstable
