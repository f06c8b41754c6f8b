"""Every implicit-GEMM tile cnn_conv2d_autotune can pin, on every desc of tests/igemm_tiles.py, bit for bit against the integer truth.

The tuner times its candidates on zeros and never looks at a result, so a tile that is wrong at some geometry can be pinned there and
cnn_conv2d_tune_import spreads it to every replica.  Here each candidate is pinned through that import call (one pass at a time, the
other pass at -1), a fresh layer is built on lattice operands (tests/exact.py: one correct bit pattern per output, in any summation
order), and forward, forward + ReLU, the prepared forward, and the four data-gradient calls must give exactly the truth.  Then the pass
runs once more on continuous operands against the C oracle (at even k, where the oracle is not defined: against the float64 arithmetic
behind the lattice truth) at the project's REL_TOL.

Whether a tile applies is read from the launch log of the plain call: it ran if a name resolves to it (igemm_tiles.tile_of); a split tile
(230 - 235) that the split rule of make_plan declines leaves another implicit-GEMM kernel in the log, and a tile whose two buffers exceed
160 KiB of LDS is refused with CNN_AMD_E_BADARG and a message that names the LDS limit -- the tuner skips both, and so does this test.
Any other refusal, a tile without a split rule that does not run, and any kernel of another family in the log are failures.

CONV_ROWS=0, FWD_RD=0 and DGRAD_RD=0 keep the specialised families off the descs; CUS is set before capi.Conv2d sizes its workspace
(tests/test_gpu_cu_counts.py).  The unpin sits in a finally per desc; no desc here is one whose launch log another test holds
(tests/test_igemm_tile_list.py).

test_coverage_conditions, at the end, asserts from what actually ran how many descs held each tile."""
import collections
import ctypes as C

import pytest

from tests import conv_route_cases as R
from tests import exact as X
from tests import igemm_tiles as G
from tests import test_gpu_exact_sums as ES
from tests.util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu

SWITCHES = (("CONV_ROWS", "0"), ("FWD_RD", "0"), ("DGRAD_RD", "0"))
FWD, DGRAD = 0, 1
PASS = ("forward", "data gradient")
PLAIN_CALL = ("forward", "backward_data")
CALLS = (("forward", "forward_relu", "forward_prepared"),
         ("backward_data", "backward_data_relu", "backward_data_prepared", "backward_data_relu_prepared"))

RAN = collections.defaultdict(set)      # (cfg, pass) -> {(desc, cus)} on which the tile ran and every call was exact
DECLINED = collections.defaultdict(set)  # (cfg, pass) -> {(desc, cus, "split rule" | "LDS")}
STAGED = collections.defaultdict(set)   # ",img" | ",img+mask" | ",img+mask+skip" -> {cfg} the log showed it for
DONE = set()                            # the (desc, cus) whose test went through all its tiles


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    arch = capi.load().cnn_amd_device_arch().decode()
    assert arch == "gfx950", f"built for gfx950, running on {arch}"
    yield torch
    print("\ndescs on which each pinned tile ran and was exact [forward, data gradient] (split tiles: (desc, CU count) pairs):")
    for c in G.CANDIDATES:
        lds = sorted(f"{PASS[m]} {R.key(d)}" for m in (FWD, DGRAD) for d, _, why in DECLINED[c, m] if why == "LDS")
        print(f"  {c}: {len(RAN[c, FWD])}, {len(RAN[c, DGRAD])}" + (f"; over the LDS limit: {', '.join(lds)}" if lds else "")
              + (f"; split accepted at {sorted((R.key(d), cus) for d, cus in RAN[c, FWD])}" if c in G.SPLIT else ""))
    for st in G.STAGINGS:
        print(f"  {st}: tiles {sorted(STAGED[st])}")


def _import(desc, entries):
    from cnn_amd import capi

    d = R.desc(desc)
    capi.check(capi.load().cnn_conv2d_tune_import(C.byref(d), (C.c_int32 * 4)(*entries)), "cnn_conv2d_tune_import")


def _export(desc):
    from cnn_amd import capi

    d, out = R.desc(desc), (C.c_int32 * 4)()
    capi.check(capi.load().cnn_conv2d_tune_export(C.byref(d), out), "cnn_conv2d_tune_export")
    return list(out)


def _pin(desc, mode, c):
    """tile c for one pass, the rule-based default (-1) for the other"""
    _import(desc, [c, -1, G.NONE, G.NONE] if mode == FWD else [-1, c, G.NONE, G.NONE])


def _unpin(desc):
    _import(desc, [-1, -1, G.NONE, G.NONE])


def _names(log):
    return [k.split("|")[0] for k in log]


def _logged(T, fn):
    """R._logged_outputs; a HIP error (a status >= CNN_AMD_E_HIP, or a failed synchronisation) is no refusal: it ends the session, as in
    tests/test_gpu_scratch_contract.py -- nothing more is started on a device that has faulted"""
    try:
        out, log = R._logged_outputs(T, fn)
    except RuntimeError as e:
        pytest.exit(f"device error in tests/test_gpu_igemm_tiles.py: {e}", returncode=3)
    if isinstance(out, int) and out >= 1000:
        from cnn_amd import capi

        pytest.exit(f"HIP error {out} in tests/test_gpu_igemm_tiles.py: {capi.load().cnn_amd_last_error().decode()}", returncode=3)
    return out, log


def _layer_calls(T, desc):
    """a fresh layer on the lattice operands, with fresh prepared buffers filled under the pin of the moment: L, {call: thunk}, truth, relu_below"""
    from cnn_amd import capi

    L, truth, relu_below = ES._layer(T, desc, X.WIDE, 1.0)
    calls = dict(R._calls(L, False))
    pf, pd = L.conv.prepared_buffers()
    pf.fill_(0x5A), pd.fill_(0x5A)
    capi.prepare_filters([L.conv], [L.w], [L.b], [pf], [pd])
    calls.update(R._prepared_calls(L, pf, pd))
    return L, calls, truth, relu_below


def _hold_pass(T, desc, mode, calls, truth, relu_below, must_run, wrong, where):
    """every call of one pass: exact bits, only implicit-GEMM kernels in the log and, with must_run = a tile, that tile in every log.
    -> False when something was wrong (all differences are appended to wrong)"""
    ok = True
    for name in CALLS[mode]:
        out, log = _logged(T, calls[name])
        if isinstance(out, int):
            wrong.append(f"{where} {name}: refused with code {out}")
            ok = False
            continue
        names = _names(log)
        strangers = [n for n in names if not G.is_igemm(n)]
        if strangers:
            wrong.append(f"{where} {name}: kernels of another family in the log: {strangers}")
            ok = False
        if must_run is not None and must_run not in [t[0] for t in map(G.tile_of, names) if t]:
            wrong.append(f"{where} {name}: the tile is not in the log: {names}")
            ok = False
        for o, t in sorted(out.items()):
            want, unit = ES._want(name, o, truth, relu_below, 1.0)
            report = X.bits_differ(ES.host(t), want, f"{where} {name}: {o}", unit)
            if report:
                wrong.append(report)
                ok = False
    return ok


_REFERENCE = {}  # desc -> (inputs, y, dx) of the continuous comparison


def _continuous(desc):
    """x, w, b, dy of tests/test_gpu_parity._conv_inputs and the reference's y and dx, once per desc.  The C oracle, except at even k:
    it transcribes the reference's walk over window CENTRES (r = (k - 1) / 2 on either side, oracle/cnn_oracle.c), which is this
    operation only for odd k -- at k = 2 it sums 1 x 1 windows and writes more outputs than the tensor holds.  There the reference is
    tests/exact.conv_f64, the float64 arithmetic behind the lattice truth (held to the oracle at odd k and to a direct loop nest at
    even k in tests/test_exact_reference.py and tests/test_igemm_tile_list.py), at the same tolerance."""
    from tests import test_gpu_parity as P

    if desc not in _REFERENCE:
        x, w, b, dy = P._conv_inputs(desc, 100)
        if desc[5] % 2:
            y_ref, _, _, dx_ref = P._oracle_conv(desc, x, w, b, dy, 100)
        else:
            y_ref, _, _, dx_ref = X.conv_f64(desc, x, w, b, dy)
        _REFERENCE[desc] = ((x, w, b, dy), y_ref, dx_ref)
    return _REFERENCE[desc]


def _hold_continuous(T, desc, mode, wrong, where):
    """the pass once more on continuous operands against the reference of _continuous, at the project's REL_TOL"""
    from cnn_amd import capi
    from tests import test_gpu_parity as P

    (x, w, b, dy), y_ref, dx_ref = _continuous(desc)
    conv = capi.Conv2d(*desc)
    try:
        if mode == FWD:
            assert_close(P.host(conv.forward(P.dev(T, x), P.dev(T, w), P.dev(T, b))), y_ref, REL_TOL, f"{where} forward vs oracle")
        else:
            assert_close(P.host(conv.backward_data(P.dev(T, dy), P.dev(T, w))), dx_ref, REL_TOL, f"{where} data grad vs oracle")
    except AssertionError as e:
        wrong.append(f"{where} continuous operands: {e}")
        return False
    return True


def _hold_tile(T, desc, cus, mode, c, wrong):
    """tile c pinned for one pass of one desc: applicability from the plain call's launch log, then every call of the pass"""
    from cnn_amd import capi

    where = f"tile {c}, {PASS[mode]}:"
    _pin(desc, mode, c)
    assert _export(desc)[:2] == ([c, -1] if mode == FWD else [-1, c])
    L = ES._layer(T, desc, X.WIDE, 1.0)[0]
    out, log = _logged(T, R._calls(L, False)[PLAIN_CALL[mode]])
    if isinstance(out, int):
        message = capi.load().cnn_amd_last_error().decode()
        if out == 1 and "of LDS" in message:  # CNN_AMD_E_BADARG: "tile needs ... B of LDS (> 160 KiB)" -- the tuner skips it too
            DECLINED[c, mode].add((desc, cus, "LDS"))
        else:
            wrong.append(f"{where} refused with code {out}: {message}")
        return
    names = _names(log)
    ran = [t for t in map(G.tile_of, names) if t and t[0] == c]
    if not ran:
        if c in G.SPLIT and all(G.is_igemm(n) for n in names) and not any(n.startswith("split_reduce/") for n in names):
            DECLINED[c, mode].add((desc, cus, "split rule"))  # (what the tuner's `pl.cfg != c` sees)
        else:
            wrong.append(f"{where} pinned and not run: {names}")
        return
    _, calls, truth, relu_below = _layer_calls(T, desc)
    ok = _hold_pass(T, desc, mode, calls, truth, relu_below, c, wrong, where)
    ok = _hold_continuous(T, desc, mode, wrong, where) and ok
    if ok:
        RAN[c, mode].add((desc, cus))
        for _, staging in ran:
            if staging:
                STAGED[staging].add(c)


@pytest.mark.parametrize("desc,cus", G.DESCS, ids=lambda v: R.key(v) if isinstance(v, tuple) else ("cus%s" % v if v else "card"))
def test_every_pinned_tile_is_exact(T, lib_option, desc, cus):
    """the ten plain descs: all 25 candidates; the split descs at their CU counts: the six split tiles (the plain tiles do not ask
    for the CU count)"""
    for name, value in SWITCHES:
        lib_option(name, value)
    if cus is not None:
        lib_option("CUS", str(cus))
    wrong = []
    try:
        for c in (G.CANDIDATES if cus is None else sorted(G.SPLIT)):
            for mode in (FWD, DGRAD):
                _hold_tile(T, desc, cus, mode, c, wrong)
    finally:
        _unpin(desc)
    assert not wrong, f"{R.key(desc)} at {'the card' if cus is None else cus}'s CUs: {len(wrong)} problem(s)\n" + "\n".join(wrong)
    DONE.add((desc, cus))


# ---- cnn_conv2d_tune_import / _export ------------------------------------------------------------------------------------------------
CONTRACT, TWIN, TUNED = G.CONTRACT, G.TWIN, G.TUNED


def _logs_and_bits(T, desc):
    """{call: (kernel names, {output: bytes})} of the seven calls of both passes on the lattice operands, each held to the truth"""
    _, calls, truth, relu_below = _layer_calls(T, desc)
    wrong, got = [], {}
    for mode in (FWD, DGRAD):
        assert _hold_pass(T, desc, mode, calls, truth, relu_below, None, wrong, R.key(desc)), "\n".join(wrong)
        for name in CALLS[mode]:
            out, log = _logged(T, calls[name])
            got[name] = (_names(log), {o: ES.host(t).tobytes() for o, t in out.items()})
    return got


def test_export_returns_what_import_pinned(lib_option):
    try:
        _import(CONTRACT, [201, 226, G.NONE, G.NONE])
        assert _export(CONTRACT) == [201, 226, G.NONE, G.NONE]
        _import(CONTRACT, [G.NONE, 215, G.NONE, G.NONE])  # (CNN_TUNE_NONE leaves an entry alone)
        assert _export(CONTRACT) == [201, 215, G.NONE, G.NONE]
        _import(CONTRACT, [G.NONE, G.NONE, G.NONE, G.NONE])
        assert _export(CONTRACT) == [201, 215, G.NONE, G.NONE]
        assert _export(TWIN) == [G.NONE] * 4  # (a table entry per geometry: the twin's stays unmeasured)
    finally:
        _unpin(CONTRACT)
    assert _export(CONTRACT) == [-1, -1, G.NONE, G.NONE]


def test_unpinned_and_unknown_tiles_run_the_rule_based_plan(T, lib_option):
    """import of -1, and of an id that is no tile (9999), give the launch log of a desc that was never pinned, and exact bits"""
    for name, value in SWITCHES:
        lib_option(name, value)
    assert _export(TWIN) == [G.NONE] * 4
    rules = {call: names for call, (names, _) in _logs_and_bits(T, TWIN).items()}
    try:
        for entry in (202, -1, 9999):
            _import(CONTRACT, [entry, entry, G.NONE, G.NONE])
            got = {call: names for call, (names, _) in _logs_and_bits(T, CONTRACT).items()}
            if entry == 202:
                for names in got.values():  # (the pin is live: what -1 and 9999 are compared with below is not an empty table's doing)
                    assert (202, "") in [G.tile_of(n) for n in names], got
                assert got != rules
            else:
                assert got == rules, (entry, got, rules)
    finally:
        _unpin(CONTRACT)


@pytest.mark.parametrize("c", [202, 226])
def test_the_option_and_the_import_pin_the_same_tile(T, lib_option, c):
    """IGEMM_CFG=c (what the tile tests of tests/test_gpu_stacks.py force) and import of c: the same launch logs, the same bits"""
    for name, value in SWITCHES:
        lib_option(name, value)
    try:
        _import(CONTRACT, [c, c, G.NONE, G.NONE])
        pinned = _logs_and_bits(T, CONTRACT)
    finally:
        _unpin(CONTRACT)
    lib_option("IGEMM_CFG", str(c))
    forced = _logs_and_bits(T, CONTRACT)
    assert pinned == forced
    assert all(any((G.tile_of(n) or (None,))[0] == c for n in names) for names, _ in pinned.values()), {k: v[0] for k, v in pinned.items()}


def test_a_measured_choice_is_a_candidate_and_exact(T):
    """a real cnn_conv2d_autotune_ws on a desc nothing else uses: what it exports is a member of the candidate list or -1, and every
    call of both passes under the pinned choice is exact"""
    from cnn_amd import capi

    lib, d = capi.load(), R.desc(TUNED)
    need = int(lib.cnn_conv2d_autotune_workspace_bytes(C.byref(d)))
    if _export(TUNED)[:2] == [G.NONE, G.NONE]:  # (measured once per process)
        assert need > 0
        scratch = T.empty(need, dtype=T.uint8, device="cuda")
        capi.check(lib.cnn_conv2d_autotune_ws(C.byref(d), capi._ptr(scratch), need, capi._stream()), "cnn_conv2d_autotune_ws")
        T.cuda.synchronize()
    fwd, dgrad, prefer_fwd, prefer_dgrad = _export(TUNED)
    assert fwd in [-1] + G.CANDIDATES and dgrad in [-1] + G.CANDIDATES, (fwd, dgrad)
    assert (prefer_fwd, prefer_dgrad) == (G.NONE, G.NONE)  # (no register-direct kernel covers a 5x5 layer)
    assert int(lib.cnn_conv2d_autotune_workspace_bytes(C.byref(d))) == 0
    got = _logs_and_bits(T, TUNED)
    for mode, c in ((FWD, fwd), (DGRAD, dgrad)):
        if c >= 0:
            for name in CALLS[mode]:
                assert any((G.tile_of(n) or (None,))[0] == c for n in got[name][0]), (name, c, got[name][0])


# ---- what the module held, from what actually ran ----------------------------------------------------------------------------------
def test_coverage_conditions():
    """Conditions, not measurements: the counts are those of a host-side restatement of make_plan's pinned branch over the descs of
    tests/igemm_tiles.py; a tile that stops applying somewhere (a new rule in make_plan, a smaller LDS budget) fails here instead of
    silently leaving the module."""
    assert DONE == set(G.DESCS), f"needs every test_every_pinned_tile_is_exact case of this run to have passed; missing: {sorted(set(G.DESCS) - DONE, key=str)}"
    plain = {(d, None) for d in G.PLAIN_DESCS}
    n = lambda c, mode: len(RAN[c, mode] & plain)
    for c in (201, 202, 206, 207, 208, 215, 216, 219, 222, 226, 0, 1):
        assert n(c, FWD) == 10 and n(c, DGRAD) == 10, (c, n(c, FWD), n(c, DGRAD), DECLINED[c, FWD], DECLINED[c, DGRAD])
    for c in (200, 225, 229):
        assert n(c, FWD) >= 8, (c, n(c, FWD), DECLINED[c, FWD])
    for c in (227, 228, 22):
        assert n(c, FWD) >= 9, (c, n(c, FWD), DECLINED[c, FWD])
    for c in (200, 225, 229, 227, 228, 22):
        assert n(c, DGRAD) == 10, (c, n(c, DGRAD), DECLINED[c, DGRAD])
    assert ((2, 20, 12, 14, 72, 2, 2, 0), None) in RAN[224, FWD], (RAN[224, FWD], DECLINED[224, FWD])
    assert n(224, DGRAD) >= 4, (n(224, DGRAD), DECLINED[224, DGRAD])
    split = {(d, c) for d, cs in G.SPLIT_DESCS.items() for c in cs}
    for c in sorted(G.SPLIT):
        assert RAN[c, FWD] & split and RAN[c, DGRAD] & split, (c, RAN[c, FWD], RAN[c, DGRAD], DECLINED[c, FWD], DECLINED[c, DGRAD])
    for mode in (FWD, DGRAD):  # ... and exactly where the split rule's arithmetic says (igemm_tiles.SPLIT_ACCEPTS), nowhere on the plain descs
        assert {pair: {c for c in G.SPLIT if pair in RAN[c, mode]} for pair in split} == G.SPLIT_ACCEPTS, PASS[mode]
        assert not any(RAN[c, mode] & plain for c in G.SPLIT), PASS[mode]
    for staging in G.STAGINGS:
        assert len(STAGED[staging]) >= 3, (staging, sorted(STAGED[staging]))
