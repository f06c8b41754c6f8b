"""The parity comparisons of tests/test_gpu_parity.py once more with the planners told the card has 1 and 5 compute units (CUS, DESIGN.md
section 10): every num_cus() site takes its "more blocks than CUs" side at the small shapes -- one workgroup walks what a whole card
shares out (1), unequal shares with ragged last units (5) -- against the same oracle, inputs and tolerance.  Nothing is compared here
that test_gpu_parity.py does not compare: each test sets CUS and calls the body of its namesake there (the oracle results are shared,
tests/test_gpu_parity._oracle_conv).  CUS is set before capi.Conv2d(...) sizes its workspace: plans, workspaces and prepared images
belong to one setting.  New here: run-to-run determinism per family, and a workspace sized for 1 CU handed to a call planned for all.

Which side each site takes (host arithmetic, read from the planners; "256" is an unpartitioned MI355X, c = the CU count).  Cases are
(B, Ci, H, W, Co, k, s, pad) of the lists named in brackets.  Where a side shows in the launch log -- an instance name, a slab count
in the tag -- test_the_switch_reaches_the_launches pins it.

site / rule                                   case                                    256                  5                     1
conv_1x1 pick_nt: tiles64 * row_blocks >= c   (2,128,28,28,256,1,2,0) [CONV] fwd      7*2 = 14: nt 2       14 >= 5: nt 4         nt 4
  (row block = 128 rows; all eight forward /  ... its data gradient (M = Ci = 128)    7*1 = 7: nt 2        nt 4                  nt 4
  dgrad launches of the four 1x1 cases have   (2,64,7,7,32,1,1,0) fwd and dgrad       2*1 = 2: nt 2        2 < 5: nt 2           nt 4
  2..14 such blocks: none reaches nt 4 at 256, two do at 5, all eight at 1)
conv_1x1 slabs: min((2c+b-1)/b, pixels/128)   (2,128,28,28,256,1,2,0), b = 2          min(256, 4) = 4      min(5, 4) = 4         1: one workgroup per tile sums all 392 pixels
conv_fwd_rd mt: tiles*ceil(mtiles/2) >= 16c   (3,32,27,27,64,3,2,0) [CONV, FWD_FAMILY] 16*1 < 4096: mt 1   16 < 80: mt 1         16 >= 16: mt 2
                                              (2,32,28,30,80,3,2,0) [FWD_FAMILY lds]  12*2 = 24: mt 1      mt 1                  24 >= 16: mt 2 (3 channel tiles: 2 + 1)
conv_fwd_rd m16: tiles*mtiles < 16c           (3,32,27,27,64,3,2,0) [CONV]            32 < 4096: m16       32 < 80: m16          32 >= 16: the LDS kernel
conv_fwd_rd bx: min(2c/cgroups, tiles/4)      (3,32,27,27,64,3,2,0), mt 2 at c = 1    -                    -                     min(2, 4) = 2: two rounds per workgroup
conv_fwd_rd parts: min(4c*waves/slices, g)    (3,32,27,27,64,3,2,0), slices 2, g = 32 min(512, 32) = 32    min(10, 32) = 10      [FWD_FAMILY m16] min(2, 32) = 2: 16 groups per wave
conv_dgrad_rd bx: min(2c/cgroups, tiles/4)    (3,16,28,27,64,3,2,0) [DGRAD_RD32],     min(512, 5) = 5      min(10, 5) = 5        2: two to three rounds per workgroup
                                              19 tiles
conv_dgrad_rd parts: min(2c*4/slices, g)      (2,32,28,30,64,3,2,0) [CONV], g = 27    min(1024, 27) = 27   min(20, 27) = 20      4: 6-7 groups per partition
  Co = 128: min(c, g)                         (5,64,13,13,128,3,2,0) [CONV], g = 16   16                   5: 3-4 groups each    1
conv_igemm small_img / CFG_D_M128:            (1,20,17,19,130,3,3,0) [CONV] fwd       2 < 512: small_img   2 < 10: small_img     2 >= 2: CFG_D_M128
  blocks(128,256) >= 2c                       ... its data gradient (M = 9 * 20)      small_img            small_img             CFG_D_M128
conv_igemm CFG_M32: blocks(32,512) >= 2c      (1,32,7,109,72,3,1,0) [ANY, ROWS_ANY=0] 2 < 512: CFG_M32_S   2 < 10: CFG_M32_S     2 >= 2: CFG_M32 (512-pixel tiles)
                                              data gradient, M = 32, 763 pixels
conv_igemm CFG_D_M128S: blocks(128,64) >= c/2 IGEMM_M128S (1,20,35,37,130,3,3,0) fwd  6 < 128: CFG_M128_S  6 >= 2: CFG_D_M128S   (2 >= 2: CFG_D_M128 first)
  (no listed case has a plane above 1024 pixels, M > 64 and few enough blocks: the case is added to the CONV list here)
conv_igemm split-Z: blocks < c,               IGEMM_SPLIT (3,40,17,17,100,3,1,0) fwd  2*2 = 4 <= 128:      2 < 5, 2 < 4 <= 6:    2 >= 1: refused
  c/2 < blocks*Z <= c + c/4                   CONV_ROWS=0, IGEMM_CFG=230 (Z = 2)      refused              split in 2
                                              ... its data gradient: 867 pixels = 3   6 <= 128: refused     3 < 5, 2 < 6 <= 6:    refused
                                              tiles, 13 chunks                                             split in 2
split-K wgrad want: c*bpc/(gy*gz) <= chunks   (3,3,38,44,72,7,2,3) [CONV]: 6 chunks,  min(256, 6) = 6      5: 3 splits of 2      1: one split walks 6 chunks
                                              bpc 2, gy*gz = 2
                                              (2,5,13,11,7,5,2,0) [CONV]: 4 chunks,   min(512, 4) = 4      min(10, 4) = 4        2 splits of 2 chunks
                                              bpc 8, gy*gz = 4
conv_stem forward gx: min(2c/co_blocks, items)(3,3,38,44,72,7,2,3) [CONV], 15 items   min(256, 15) = 15    5: 3 items each       1: 15 items
conv_stem wgrad gx (= slab count)             (2,3,22,264,72,7,2,3) [CONV], 44 items  44                   5                     1
conv_direct wave_grid: min(need, 32c)         (2,3,224,224,16,3,2,0) [first block],   97 < 8192            97 < 160              32: each wave walks 3-4 items
                                              386 items / 4 waves = 97 workgroups
                                              (conv_direct_fwd: 222 rows / 4 = 56)    56                   56                    32
conv_direct wgrad slabs: min(items, 2c)       (2,3,224,224,16,3,2,0), 386 items       min(386, 512) = 386  10: 39 items each     2: 193 items each
  (conv_wgrad_pk, + pool / + poolm; runs    (3,3,37,41,16,3,2,0), 18 items          18                   10: 2 items, last 0   2: 9 items each
  only with WG_WIN=0: conv_wgrad_win takes every geometry first, so the first-block bodies are repeated with it in the tests
  test_first_layer_packed_weight_gradient_*)
conv_wgrad_win grid: min(strips/8, c)         (2,3,224,224,16,3,2,0), 448 strips      56, lockstep         5: 12 strips a wave,  1: 56 strips a wave, lockstep
                                                                                                           480 != 448: ragged,
                                                                                                           no lockstep
pool row_grid: min(rows/4, 16c)               (2,16,111,111) k2 s2 forward, 1760 rows 440 < 4096           80: 5.5 rounds        16: 27.5 rounds
conv_rows tall units (cost rule)              (3,32,28,56,48,3,1,1) [TALL] baseline   14 > 8: short        28 > 24: short        84 < 96: tall
split_units(units, c / ntiles)                (2,64,56,56,64,3,1,1) [ROWS], 14 units  14 x 1               5 x 3 (last: 2)       1 x 14 (what ROWS_BLOCKS=1 forces)
  conv_rows / _any / _s2 / wgrad_sp*: the families' own *_BLOCKS overrides still win; at c = 1 the default walk equals their "=1" runs
wgrad_rd want: 2c / colblocks                 (3,130,7,7,96,3,1,1) [RD], 24 colblocks 21 pixel ranges      1                     1
stream_grid / slab reductions: min(need, 8c)  every element-wise launch of the above is a grid-stride loop over 8 (40) workgroups

(pick_nt: a row block is kMT = 16 rows x 8 waves = 128 rows, so the small 1x1 cases have 2..14 blocks, not the 4..112 of 16-row blocks.)"""
import ctypes as C

import numpy as np
import pytest

from tests import conv_route_cases as R
from tests import guarded
from tests import test_gpu_parity as P
from tests.util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu

IGEMM_M128S = (1, 20, 35, 37, 130, 3, 3, 0)  # the table's CFG_D_M128S row: 1295-pixel planes, 11 x 12 outputs, two 128-row tiles
IGEMM_SPLIT = (3, 40, 17, 17, 100, 3, 1, 0)  # ... its split-Z row: 675 output pixels = two 416-pixel tiles, five 8-channel chunks


@pytest.fixture(scope="module")
def T():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from cnn_amd import capi

    arch = capi.load().cnn_amd_device_arch().decode()
    assert arch == "gfx950", f"built for gfx950, running on {arch}"
    return torch


@pytest.fixture(params=[1, 5], ids=lambda n: f"cus{n}")
def cus(request, lib_option):
    """the planners' CU count for this test (restored by lib_option); every test asks for it in front of anything that builds a Conv2d"""
    lib_option("CUS", str(request.param))
    return request.param


def _cases(test, arg="case"):
    """the values an existing test is parametrised with"""
    for m in test.pytestmark:
        if m.name == "parametrize" and m.args[0] == arg:
            return list(m.args[1])
    raise KeyError(arg)


_id = lambda c: "B%d_%dx%dx%d_to%d_k%ds%dp%d" % c
_small = lambda shapes: [s for s in shapes if s not in ((256, 224, 224), (16, 224, 224))]
_shape_id = lambda s: "B%d_%dx%d" % s


@pytest.mark.parametrize("case", P.CONV_CASES + [IGEMM_M128S], ids=_id)
def test_conv2d_mfma_vs_oracle(T, cus, case):
    P.test_conv2d_mfma_vs_oracle(T, case)


def test_conv2d_implicit_gemm_split_tile_vs_oracle(T, cus, lib_option):
    """the split-Z rule of conv_igemm.hip's pinned tiles: taken at 5 CUs, refused at 1 (and at 256) -- same comparisons"""
    lib_option("CONV_ROWS", "0")
    lib_option("IGEMM_CFG", "230")
    P.test_conv2d_mfma_vs_oracle(T, IGEMM_SPLIT)


@pytest.mark.parametrize("slow", [False, True], ids=["pipelined", "guarded"])
@pytest.mark.parametrize("case", _cases(P.test_conv2d_wgrad_register_direct), ids=_id)
def test_conv2d_wgrad_register_direct(T, cus, case, slow, lib_option):
    P.test_conv2d_wgrad_register_direct(T, case, slow, lib_option)


@pytest.mark.parametrize("unit", [0, 1], ids=["dma16", "dma4"])
@pytest.mark.parametrize("case", P.SP_CASES, ids=_id)
def test_conv2d_wgrad_small_planes(T, cus, case, unit, lib_option):
    rep = P._wgrad_small_planes(T, case, unit, lib_option)
    assert any(k.startswith("wgrad_sp<") for k in rep), list(rep)  # (WGRAD_SP=1 picks the family at any CU count)


@pytest.mark.parametrize("case", P.SP2_CASES, ids=_id)
def test_conv2d_wgrad_small_planes_stride2(T, cus, case, lib_option):
    rep = P._wgrad_small_planes_stride2(T, case, lib_option)
    assert any(k.startswith("wgrad_sp2<") for k in rep), list(rep)


@pytest.mark.parametrize("case", P.SPA_CASES, ids=_id)
def test_conv2d_wgrad_any_size_vs_oracle(T, cus, case, lib_option):
    rep = P._wgrad_any_size(T, case, lib_option)
    assert any(k.startswith("wgrad_sp_any<") for k in rep), list(rep)


@pytest.mark.parametrize("case", P.ROWS_CASES, ids=_id)
def test_conv2d_row_kernel_vs_oracle(T, cus, case, lib_option):
    default, walk = P._row_kernel(T, case, lib_option)
    # (whether the row kernels cover a layer does not depend on the CU count; their tile and unit height may: not asserted)
    assert sum(n.startswith("conv_rows<") for n in default) == 2, default
    assert sum(n.startswith("conv_rows<") for n in walk) == 4, walk


@pytest.mark.parametrize("case", P.ANY_CASES, ids=_id)
def test_conv2d_row_kernel_any_width_vs_oracle(T, cus, case, lib_option):
    for names in P._row_kernel_any_width(T, case, lib_option):
        assert sum(n.startswith("conv_rows_any<") for n in names) == (4 if case[1] >= 16 else 2), names


@pytest.mark.parametrize("case", P.TALL_CASES, ids=_id)
def test_conv2d_row_kernel_tall_units_vs_oracle(T, cus, case, lib_option):
    for names in P._row_kernel_tall_units(T, case, lib_option):
        tall = [n for n in names if n.startswith("conv_rows<") and ",r14>" in n or ",r7>" in n]
        assert len(tall) == 4, names  # (ROWS_TALL=2 forces them at any CU count)


@pytest.mark.parametrize("case", P.STEM_DGRAD_CASES, ids=_id)
def test_conv2d_stem_data_gradient_packed_vs_oracle(T, cus, case, lib_option):
    P.test_conv2d_stem_data_gradient_packed_vs_oracle(T, case, lib_option)  # (conv_dgrad_thin.hip asks for no CU count: same kernels, its names asserted)


@pytest.mark.parametrize("case", P.S2_CASES, ids=_id)
def test_conv2d_stride2_row_kernel_vs_oracle(T, cus, case, lib_option):
    for names in P._stride2_row_kernel(T, case, lib_option):
        assert sum(n.startswith("conv_s2<") for n in names) == 4, names


@pytest.mark.parametrize("family", ["lds", "m16"])
@pytest.mark.parametrize("case", P.FWD_FAMILY_CASES, ids=_id)
def test_conv2d_forward_kernel_families(T, cus, case, family, lib_option):
    P.test_conv2d_forward_kernel_families(T, case, family, lib_option)


@pytest.mark.parametrize("case", _cases(P.test_conv2d_dgrad_register_direct_opt_in_tiles), ids=_id)
def test_conv2d_dgrad_register_direct_opt_in_tiles(T, cus, case, lib_option):
    P.test_conv2d_dgrad_register_direct_opt_in_tiles(T, case, lib_option)


def test_conv2d_combined_backward_matches_separate_calls(T, cus):
    P.test_conv2d_combined_backward_matches_separate_calls(T)


def test_prepared_filters_match_plain_calls(T, cus):
    P.test_prepared_filters_match_plain_calls(T)


@pytest.mark.parametrize("shape,k,step", _cases(P.test_maxpool_bit_exact, "shape,k,step"))
def test_maxpool_bit_exact(T, cus, shape, k, step):
    P.test_maxpool_bit_exact(T, shape, k, step)


@pytest.mark.parametrize("shape,k,step", _cases(P.test_maxpool_backward_relu_fusion_is_bit_identical, "shape,k,step"))
def test_maxpool_backward_relu_fusion_is_bit_identical(T, cus, shape, k, step):
    P.test_maxpool_backward_relu_fusion_is_bit_identical(T, shape, k, step)


@pytest.mark.parametrize("shape", _small(_cases(P.test_conv_relu_maxpool_fusion_is_bit_identical, "shape")), ids=_shape_id)
@pytest.mark.parametrize("prepared", [False, True], ids=["plain", "prepared"])
def test_conv_relu_maxpool_fusion_is_bit_identical(T, cus, shape, prepared):
    P.test_conv_relu_maxpool_fusion_is_bit_identical(T, shape, prepared)


@pytest.mark.parametrize("shape", _small(_cases(P.test_conv_backward_from_pooled_domain_is_bit_identical, "shape")), ids=_shape_id)
def test_conv_backward_from_pooled_domain_is_bit_identical(T, cus, shape):
    P.test_conv_backward_from_pooled_domain_is_bit_identical(T, shape)


@pytest.mark.parametrize("shape", _small(_cases(P.test_packed_pool_mask_block_is_bit_identical, "shape")), ids=_shape_id)
def test_packed_pool_mask_block_is_bit_identical(T, cus, shape):
    P.test_packed_pool_mask_block_is_bit_identical(T, shape)


@pytest.mark.parametrize("shape", _small(_cases(P.test_first_layer_weight_gradient_sgd_prepare_fusion_is_bit_identical, "shape")), ids=_shape_id)
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_first_layer_weight_gradient_sgd_prepare_fusion_is_bit_identical(T, cus, shape, scale):
    P.test_first_layer_weight_gradient_sgd_prepare_fusion_is_bit_identical(T, shape, scale)


def test_the_switch_reaches_the_launches(T, cus):
    """the launch log of two weight gradients whose tag carries the slab count: the table's conv_1x1 row (4 / 4 / 1 slabs) and
    wgrad_sp's split_units over the 35 sample pairs of (70, 64, 7, 7, 64, 3, 1, 1) -- no more pixel ranges than the pretend card has CUs"""
    from cnn_amd import capi

    def slabs(case, kernel):
        x, _, _, dy = P._conv_inputs(case, 100)
        conv = capi.Conv2d(*case)
        xd, dyd = P.dev(T, x), P.dev(T, dy)
        capi.kernel_timing(1)
        conv.backward_weight(xd, dyd, float(case[0]))
        T.cuda.synchronize()
        keys = [k for k in capi.kernel_timing_report() if k.startswith(kernel)]
        capi.kernel_timing(0)
        assert len(keys) == 1, keys
        return int(keys[0].rsplit("slabs", 1)[1])

    assert slabs(P.CONV_CASES[29], "conv_1x1/wgrad") == {1: 1, 5: 4}[cus]
    assert 1 <= slabs(P.SP_CASES[12], "wgrad_sp<") <= cus  # (35 on a whole card)

    def forward_kernels(case):
        x, w, b, _ = P._conv_inputs(case, 100)
        conv = capi.Conv2d(*case)
        xd, wd, bd = P.dev(T, x), P.dev(T, w), P.dev(T, b)
        capi.kernel_timing(1)
        conv.forward(xd, wd, bd)
        T.cuda.synchronize()
        names = [k.split("|")[0] for k in capi.kernel_timing_report()]
        capi.kernel_timing(0)
        return names

    # the table's conv_fwd_rd mt / m16 rows, its tall-unit row and its split-Z row, by the instances' launch-log names
    assert forward_kernels(P.CONV_CASES[6]) == [{1: "conv_fwd_rd<2,32,2>/fwd", 5: "conv_fwd_rd<2,32,m16>/fwd"}[cus]]
    assert {1: "conv_rows<56,1,64,r14>/fwd", 5: "conv_rows<56,1,64>/fwd"}[cus] in forward_kernels(P.TALL_CASES[1])
    with capi.option("CONV_ROWS", "0"), capi.option("IGEMM_CFG", "230"):
        assert ("split_reduce/fwd" in forward_kernels(IGEMM_SPLIT)) == (cus == 5)


# one desc per kernel family of tests/conv_route_cases.HAND_PICKED: first layer, stem, 1x1, thin input, the three stride-2 reference
# layers' families, per-width and runtime-width row kernels, stride-1 register-direct, a pad-1 stage entry, k = 5, stride 3
DETERMINISM_CASES = [R.HAND_PICKED[i] for i in (0, 3, 5, 7, 9, 11, 14, 17, 21, 23, 26, 27)]


@pytest.mark.parametrize("case", DETERMINISM_CASES, ids=lambda c: R.key(c))
def test_two_runs_under_one_cu_count_are_bit_identical(T, cus, case):
    """forward, forward + ReLU, both gradients and the data gradient with ReLU': the same bytes from two runs (a plan with several
    rounds per workgroup or several slabs per sum must not depend on which workgroup comes first)"""
    layer = R._Layer(T, case, 9100)
    calls = {n: f for n, f in R._calls(layer, False).items() if "/" not in n}
    assert sorted(calls) == ["backward_data", "backward_data_relu", "backward_weight", "forward", "forward_relu"]
    for name, fn in calls.items():
        first, again = ({k: R._sha(t) for k, t in fn().items()} for _ in range(2))
        assert first == again, name


@pytest.mark.parametrize("shape", _small(_cases(P.test_conv_backward_from_pooled_domain_is_bit_identical, "shape")), ids=_shape_id)
def test_first_layer_packed_weight_gradient_from_pooled_domain(T, cus, shape, lib_option):
    """conv_direct.hip's own weight gradient (conv_wgrad_pk and its +pool / +poolm forms), which runs where conv_wgrad_win.hip is switched
    off: min(items, 2 * cus) slabs, every workgroup a contiguous range of 64-pixel items (the table's conv_direct wgrad row)"""
    lib_option("WG_WIN", "0")
    P.test_conv_backward_from_pooled_domain_is_bit_identical(T, shape)


@pytest.mark.parametrize("shape", _small(_cases(P.test_first_layer_weight_gradient_sgd_prepare_fusion_is_bit_identical, "shape")), ids=_shape_id)
def test_first_layer_packed_weight_gradient_sgd_prepare_fusion(T, cus, shape, lib_option):
    lib_option("WG_WIN", "0")
    P.test_first_layer_weight_gradient_sgd_prepare_fusion_is_bit_identical(T, shape, 0.5)


def test_first_layer_packed_weight_gradient_vs_oracle(T, cus, lib_option):
    from cnn_amd import capi

    lib_option("WG_WIN", "0")
    case = P.CONV_CASES[5]
    x, _, _, dy = P._conv_inputs(case, 100)
    xd, dyd = P.dev(T, x), P.dev(T, dy)
    capi.kernel_timing(1)
    capi.Conv2d(*case).backward_weight(xd, dyd, float(case[0]))
    T.cuda.synchronize()
    names = [k.split("|")[0] for k in capi.kernel_timing_report()]
    capi.kernel_timing(0)
    assert "conv_wgrad_pk<3,16,3,2>" in names, names
    P.test_conv2d_mfma_vs_oracle(T, case)


# one desc per slab family of cnn_conv2d_backward_weight (conv_wgrad.hip: kSlabFamilies, then the split-K kernel), all of CONV_CASES:
# family -> (case, the launch-log prefix of the family's kernel)
SLAB_CASES = {"direct": (P.CONV_CASES[5], "conv_wgrad_win<"), "1x1": (P.CONV_CASES[29], "conv_1x1/wgrad"), "sp": (P.CONV_CASES[16], "wgrad_sp<"),
              "os": (P.CONV_CASES[7], "conv_wgrad_os<"), "rd": (P.CONV_CASES[6], "wgrad_rd<"), "stem": (P.CONV_CASES[22], "conv_stem_wgrad<"),
              "split-K": (P.CONV_CASES[4], "wgrad_kernel<")}


@pytest.mark.parametrize("poison", guarded.POISONS)
@pytest.mark.parametrize("family", sorted(SLAB_CASES))
def test_workspace_sized_for_one_cu_is_refused_or_enough(T, family, poison, lib_option):
    """A workspace of exactly cnn_conv2d_workspace_bytes(desc) under CUS=1, between guard zones, handed to cnn_conv2d_backward_weight with
    CUS unset (more slabs wanted than it holds): CNN_AMD_E_WORKSPACE, or success with the oracle's gradients; no byte outside it changes.
    That the desc belongs to the family it is listed under shows in the launch log of the two calls whose workspace was sized for them:
    under CUS=1 with that workspace, and with CUS unset and the full one"""
    from cnn_amd import capi

    case, prefix = SLAB_CASES[family]
    lib, d = capi.load(), R.desc(case)
    lib_option("CUS", "1")
    small = int(lib.cnn_conv2d_workspace_bytes(C.byref(d)))
    lib_option("CUS", None)
    full = int(lib.cnn_conv2d_workspace_bytes(C.byref(d)))
    assert 0 < small <= full
    x, w, b, dy = P._conv_inputs(case, 100)
    _, gw_ref, gb_ref, _ = P._oracle_conv(case, x, w, b, dy, 100)
    xd, dyd = P.dev(T, x), P.dev(T, dy)

    def call(told, what):
        """-> (status, the kernels launched in front of the slab reduction)"""
        ws = guarded.scratch(full, told_bytes=told, poison=poison, name=f"ws of {told} bytes, {what} ({small} for 1 CU, {full} for the card)")
        keep = []
        gw, gb = guarded.output(w.shape, poison, keep, "gw"), guarded.output(b.shape, poison, keep, "gb")
        capi.kernel_timing(1)
        rc = lib.cnn_conv2d_backward_weight(C.byref(d), capi._ptr(xd), capi._ptr(dyd), capi._ptr(gw), capi._ptr(gb), float(case[0]),
                                            capi._ptr(ws.view), told, capi._stream())
        T.cuda.synchronize()
        names = [k.split("|")[0] for k in capi.kernel_timing_report()]
        capi.kernel_timing(0)
        assert rc in (0, 2), (what, rc, lib.cnn_amd_last_error().decode())  # CNN_AMD_OK | CNN_AMD_E_WORKSPACE
        assert not guarded.check([ws] + keep), what
        if rc == 0:
            assert_close(P.host(gw), gw_ref, REL_TOL, f"weight grad, {what}")
            assert_close(P.host(gb), gb_ref, REL_TOL, f"bias grad, {what}")
        return rc, [n for n in names if not n.startswith(("slab_reduce", "bias_grad"))]

    lib_option("CUS", "1")
    rc, names = call(small, "sized and called under CUS=1")
    assert rc == 0 and len(names) == 1 and names[0].startswith(prefix), (rc, names)
    lib_option("CUS", None)
    rc, names = call(full, "sized and called for the whole card")
    assert rc == 0 and len(names) == 1 and names[0].startswith(prefix), (rc, names)
    rc, names = call(small, "sized under CUS=1, called for the whole card")
    assert (rc == 2 and not names) or (rc == 0 and len(names) == 1), (rc, names)  # (the family, or one behind it that the buffer holds)


