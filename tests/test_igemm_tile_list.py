"""tests/igemm_tiles.py against the source it restates, and its descs against the conditions tests/test_gpu_igemm_tiles.py relies on
(no device needed)."""
import os
import re

import numpy as np

from tests import conv_route_cases as R
from tests import exact as X
from tests import igemm_tiles as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "cnn_amd", "csrc", "conv_igemm.hip")


def _descs_in(module):
    """every 8-integer tuple (a desc, flags dropped) anywhere in a module's lists, tuples and dicts"""
    found = set()

    def walk(v, depth=0):
        if isinstance(v, tuple) and len(v) in (8, 9) and all(isinstance(i, int) and not isinstance(i, bool) for i in v):
            found.add(tuple(v[:8]))
        elif isinstance(v, (list, tuple, set, frozenset)) and depth < 6:
            for i in v:
                walk(i, depth + 1)
        elif isinstance(v, dict) and depth < 6:
            for k, i in v.items():
                walk(k, depth + 1)
                walk(i, depth + 1)

    for name, v in vars(module).items():
        if not name.startswith("__"):
            walk(v)
    return found


def test_candidates_are_the_tuners():
    """a candidate added to kTuneCandidates later cannot go untested: the list here is the source's"""
    src = open(SOURCE).read()
    m = re.search(r"const\s+int\s+kTuneCandidates\[\]\s*=\s*\{([^}]*)\}", src)
    assert m, "kTuneCandidates not found in conv_igemm.hip"
    listed = [int(v) for v in m.group(1).split(",")]
    assert listed == [-1] + G.CANDIDATES
    assert len(set(G.CANDIDATES)) == len(G.CANDIDATES) == 25
    assert sorted(G.KERNEL) == sorted(G.CANDIDATES)
    assert set(G.SPLIT) <= set(G.CANDIDATES)
    m = re.search(r"#define\s+CNN_TUNE_NONE\s+\((-?\d+)\s*-\s*1\)", open(os.path.join(ROOT, "include", "cnn_amd.h")).read())
    assert m and int(m.group(1)) - 1 == G.NONE


def test_kernel_names_are_the_tables():
    """KERNEL[cfg] against the kernel and the six template arguments run_plan launches for the tile's row of kTiles (the enum gives the
    number of each name), the ",k/Z" suffix from the row's Z; and the table has one row per enum value"""
    src = open(SOURCE).read()
    ids, rows = G.source_enum(src), G.source_tiles(src)
    assert len(set(ids.values())) == len(ids)
    assert sorted(ids[name] for name, _ in rows) == sorted(ids.values()), "kTiles and the enum do not hold the same ids"
    # how a row becomes a launch: the two launcher templates and their arguments, S from CK and the MFMA's k-step
    flat = re.sub(r"\s+", " ", src)
    assert "if constexpr (t.dma) return launch_dma<t.MF, t.MA, t.NB, t.WM, t.WN, t.S(), t.img>(pl, s, d);" in flat
    assert "else return launch_cfg<t.MF, t.MA, t.NB, t.WM, t.WN, t.CK>(pl, s, d);" in flat
    assert "constexpr int S() const { return CK / kstep(); }" in flat
    assert "constexpr int kstep() const { return MF == 32 ? Acc<32>::kStep : Acc<16>::kStep; }" in flat
    ksteps = re.findall(r"struct Acc<(\d+)> \{.*?static constexpr int kStep = (\d+);", src, re.S)
    assert sorted(ksteps) == [("16", "4"), ("32", "2")]
    assert "switch (pl.cfg)" not in src and "case CFG_" not in src
    seen = G.source_table(src)
    for cfg in G.CANDIDATES:
        assert seen[cfg]["Z"] == G.SPLIT.get(cfg, 1), cfg
        assert G.KERNEL[cfg] == G.kernel_of(seen[cfg]), (cfg, G.KERNEL[cfg], G.kernel_of(seen[cfg]))
    for cfg, row in seen.items():  # (what the C++ static_asserts hold, for the rows the tuner does not try as well)
        assert row["Z"] >= 1 and row["CK"] % {32: 2, 16: 4}[row["MF"]] == 0 and (row["dma"] or (row["Z"] == 1 and not row["img"])), cfg


def test_names_resolve_to_one_tile():
    for cfg, prefix in G.KERNEL.items():
        close = "" if prefix.endswith(">") else ">"
        for mode in ("/fwd", "/fwd+relu", "/dgrad", "/dgrad+relu"):
            assert G.tile_of(prefix + close + mode + "|B1 Ci1") == (cfg, "")
            if not prefix.endswith(">") and cfg not in G.SPLIT:
                for st in G.STAGINGS:
                    assert G.tile_of(prefix + st + ">" + mode) == (cfg, st)
    assert G.tile_of("igemm_dma_kernel<16,1,4,1,4,1>/fwd") is None  # (a rule-based tile that is no candidate)
    assert G.tile_of("igemm_prep_weights/fwd") is None and G.is_igemm("igemm_prep_weights/fwd")
    assert G.is_igemm("split_reduce/dgrad+relu") and not G.is_igemm("conv_rows<56,1,64>/fwd")


def test_descs_stay_on_the_lattice():
    """every partial sum of every output of every desc is an fp32 integer (tests/exact.py)"""
    assert len(G.PLAIN_DESCS) == 10 and len(G.DESCS) == 17 and len(set(G.DESCS)) == 17
    for desc in [d for d, _ in G.DESCS] + [G.CONTRACT, G.TWIN, G.TUNED]:
        assert X.headroom(desc) < X.LIMIT, (desc, X.headroom(desc))


def test_descs_are_nobody_elses():
    """the tune table is per process: a pin must not land on a desc whose golden launch log another test holds"""
    from tests import stream_order_cases
    from tests import test_gpu_parity as P

    held = {tuple(c[:8]) for c in R.HAND_PICKED} | set(P.CONV_CASES) | set(P.RD_CASES) | _descs_in(stream_order_cases)
    assert len(held) > 40
    mine = [d for d, _ in G.DESCS] + [G.CONTRACT, G.TWIN, G.TUNED]
    assert len(set(mine)) == 12 + 3
    for desc in mine:
        assert desc not in held, desc


def test_float64_reference_is_the_operation_at_even_k():
    """tests/exact.conv_f64 is the reference of the continuous comparison where the C oracle is not defined (even k: its window is
    2 * ((k - 1) / 2) + 1 wide).  Held here to the definition written as a loop nest, on lattice operands (exact in float64) at k = 2
    and k = 4 with stride and padding, and to the oracle on continuous operands at an odd k, where both are defined."""
    from tests import test_gpu_parity as P
    from tests.util import rel_err

    for case in [(2, 3, 6, 7, 4, 2, 2, 0), (1, 2, 5, 6, 3, 4, 2, 1), (2, 2, 4, 5, 3, 2, 1, 1)]:
        B, Ci, H, W, Co, k, s, pad, Ho, Wo = X.geometry(case)
        x, w, b, dy = X.lattice_inputs(case, 5)
        xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
        y, dxp = np.zeros((B, Co, Ho, Wo)), np.zeros_like(xp)
        for n in range(B):
            for co in range(Co):
                for p in range(Ho):
                    for q in range(Wo):
                        y[n, co, p, q] = b[co] + float((xp[n, :, p * s:p * s + k, q * s:q * s + k] * w[co]).sum())
                        dxp[n, :, p * s:p * s + k, q * s:q * s + k] += np.float64(dy[n, co, p, q]) * w[co]
        got = X.conv_f64(case, x, w, b, dy)
        assert np.array_equal(got[0], y), case
        assert np.array_equal(got[3], dxp[:, :, pad:pad + H, pad:pad + W]), case
    case = G.PLAIN_DESCS[0]
    x, w, b, dy = P._conv_inputs(case, 100)
    y_ref, _, _, dx_ref = P._oracle_conv(case, x, w, b, dy, 100)
    y, _, _, dx = X.conv_f64(case, x, w, b, dy)
    assert rel_err(y_ref, y) < 1e-6 and rel_err(dx_ref, dx) < 1e-6, (rel_err(y_ref, y), rel_err(dx_ref, dx))
