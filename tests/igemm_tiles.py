"""The implicit-GEMM tiles cnn_conv2d_autotune can pin, their launch-log names and the descs they are held on (no device needed).

cnn_conv2d_autotune times kTuneCandidates (cnn_amd/csrc/conv_igemm.hip) on all-zero buffers and pins the fastest tile per geometry and
pass without looking at a result; cnn_conv2d_tune_import spreads the choice to every replica.  tests/test_gpu_igemm_tiles.py pins every
candidate through the import call on every desc below and holds what it computes to the integer truth of tests/exact.py;
tests/test_igemm_tile_list.py keeps this module in step with the source."""
import os
import re

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cnn_amd", "csrc", "conv_igemm.hip")
TILE_FIELDS = ("dma", "MF", "MA", "NB", "WM", "WN", "CK", "img", "Z")


def source_enum(src=None):
    """{CFG_ name: number} of the tile enum in conv_igemm.hip"""
    src = open(SOURCE).read() if src is None else src
    enum = re.search(r"enum\s*\{\s*(CFG_M128_L\s*=.*?)\};", src, re.S).group(1)
    enum = re.sub(r"/\*.*?\*/", "", enum)
    value, ids = -1, {}
    for item in enum.split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            item, v = (s.strip() for s in item.split("="))
            value = int(v)
        else:
            value += 1
        assert item not in ids, item
        ids[item] = value
    return ids


def source_tiles(src=None):
    """[(CFG_ name, {field: value})] of the rows of kTiles in conv_igemm.hip, in the table's order (duplicates kept)"""
    src = open(SOURCE).read() if src is None else src
    body = re.search(r"constexpr\s+Tile\s+kTiles\[\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    rows = re.findall(r"\{([^{}]*)\}", body)
    assert re.sub(r"\{[^{}]*\}|[\s,]", "", body) == "", "kTiles holds something that is no row"
    out = []
    for row in rows:
        cells = [c.strip() for c in row.split(",")]
        assert len(cells) == 1 + len(TILE_FIELDS), row
        value = {"true": True, "false": False}
        out.append((cells[0], {f: value[c] if c in value else int(c) for f, c in zip(TILE_FIELDS, cells[1:])}))
    return out


def source_table(src=None):
    """{id: row} of kTiles"""
    ids = source_enum(src)
    return {ids[name]: row for name, row in source_tiles(src)}


def kernel_of(row):
    """the launch-log name of a row's kernel up to where the staging mode follows (the form of KERNEL below): igemm_dma_kernel<MF, MA, NB,
    WM, WN, CK / k-step of the MFMA [, k/Z] or igemm_kernel<MF, MA, NB, WM, WN, CK> -- what launch_row in conv_igemm.hip instantiates"""
    head = "%d,%d,%d,%d,%d," % tuple(row[f] for f in ("MF", "MA", "NB", "WM", "WN"))
    if not row["dma"]:
        return _LDS + head + "%d>" % row["CK"]
    kstep = {32: 2, 16: 4}[row["MF"]]
    assert row["CK"] % kstep == 0
    return _DMA + head + "%d" % (row["CK"] // kstep) + (",k/%d" % row["Z"] if row["Z"] > 1 else "")


# kTuneCandidates without -1 (the rule-based default)
CANDIDATES = [200, 201, 206, 207, 208, 226, 222, 224, 215, 216, 219, 225, 0, 1, 22, 227, 202, 228, 229, 230, 231, 232, 233, 234, 235]
SPLIT = {230: 2, 231: 4, 232: 8, 233: 2, 234: 4, 235: 8}  # the wide tiles with the channel range split in Z
NONE = -2 ** 31  # CNN_TUNE_NONE (include/cnn_amd.h)

_DMA, _LDS = "igemm_dma_kernel<", "igemm_kernel<"
# the launch-log name of each tile up to where the staging mode follows, restated from the rows of kTiles that run_plan dispatches over
KERNEL = {
    200: _DMA + "32,4,1,1,8,4", 201: _DMA + "32,2,1,1,8,4", 202: _DMA + "32,2,2,1,4,4",
    206: _DMA + "32,4,1,1,8,2", 207: _DMA + "32,2,2,1,4,2", 208: _DMA + "32,2,1,1,4,2",
    215: _DMA + "32,1,1,1,4,4", 216: _DMA + "32,1,1,1,4,2", 219: _DMA + "32,2,1,2,2,2",
    222: _DMA + "32,1,1,1,4,8", 224: _DMA + "32,2,1,2,2,8", 225: _DMA + "32,2,1,1,4,8", 226: _DMA + "32,2,1,1,4,4",
    227: _DMA + "32,2,2,1,8,4",
    228: _DMA + "16,2,13,2,4,2", 233: _DMA + "16,2,13,2,4,2,k/2", 234: _DMA + "16,2,13,2,4,2,k/4", 235: _DMA + "16,2,13,2,4,2,k/8",
    229: _DMA + "16,2,13,4,2,2", 230: _DMA + "16,2,13,4,2,2,k/2", 231: _DMA + "16,2,13,4,2,2,k/4", 232: _DMA + "16,2,13,4,2,2,k/8",
    0: _LDS + "32,4,1,1,4,8>", 1: _LDS + "32,2,1,2,2,8>", 22: _LDS + "32,2,1,2,2,16>",
}
STAGINGS = (",img", ",img+mask", ",img+mask+skip")  # whole-image staging as the name shows it (rows: nothing)
_TAIL = re.compile(r"(,img(\+mask(\+skip)?)?)?>/")


def tile_of(name):
    """(cfg, staging) of an implicit-GEMM launch-log name ("" for row staging), None for any other kernel.  A name belongs to the tile
    whose KERNEL entry it starts with and behind which only the staging mode and the pass follow (so 228 does not claim 233's ",k/2")."""
    name = name.split("|")[0]
    for cfg, prefix in KERNEL.items():
        if not name.startswith(prefix):
            continue
        rest = name[len(prefix) - 1:] if prefix.endswith(">") else name[len(prefix):]
        m = _TAIL.match(rest)
        if m:
            return cfg, m.group(1) or ""
    return None


def is_igemm(name):
    """any kernel of conv_igemm.hip's forward / data-gradient path: a tile, the filter re-arrangement or the split reduction"""
    return name.startswith((_DMA, _LDS, "igemm_prep_weights/", "split_reduce/"))


# (B, Ci, H, W, Co, k, s, pad) -> the CU counts it runs at (None: the card's)
PLAIN_DESCS = [
    (3, 6, 10, 10, 40, 3, 1, 1),     # padded rows of 10 floats: 16-byte row DMA with a ragged tail of 2; whole-image + mask on the small-image tiles; a 6-channel last chunk; tiles span images
    (3, 5, 13, 11, 7, 5, 2, 0),      # 25 taps forward (some tiles exceed LDS and must be refused cleanly); stride-2 data gradient with tap skipping
    (2, 20, 17, 19, 130, 3, 3, 0),   # stride 3: a 1-tap data-gradient window; M = 130: two 128-row blocks with 2 live rows in the second
    (1, 16, 36, 40, 48, 3, 1, 0),    # plane above 1024: row staging for every tile; unpadded, W % 4 == 0: run mode 1 forward; ragged data gradient (rows of 38)
    (1, 24, 34, 36, 72, 3, 1, 1),    # padded, W % 4 == 0: run mode 3 without a tail; C = 24: a half-full chunk for the 16-channel tiles
    (2, 12, 37, 41, 20, 3, 2, 1),    # stride 2, pad 1, 41-wide plane (tail 1); the data gradient reads a 19x21 plane with whole-image staging
    (7, 8, 9, 9, 136, 3, 1, 1),      # 567 pixels over 7 images: every 64/128-pixel tile spans 2-3 images; M = 136
    (1, 12, 30, 30, 40, 3, 1, 1),    # 900-pixel plane, C % 8 != 0: the whole-image tiles need more than 8 DMA descriptors per wave (the non-precomputed path)
    (2, 20, 12, 14, 72, 2, 2, 0),    # k = 2 (4 taps): of these nine the only forward geometry at which 224 fits LDS
    # the issue that asked for this list counts ten non-split descs and names nine; the tenth is this module's: 35 output pixels, fewer
    # than the narrowest tile holds (one workgroup column, 29 to 797 dead pixels in it), rows of 5 floats (one 16-byte unit and a ragged
    # tail of 1), a 1-channel last chunk, M = 33 (one live row in the second 32-row block)
    (1, 9, 7, 5, 33, 3, 1, 1),
]
SPLIT_DESCS = {
    (2, 124, 9, 9, 124, 3, 1, 1): (2, 4, 8, 14),   # one wide tile; 124 channels: 16 chunks with a 4-channel last one
    (3, 128, 14, 14, 128, 3, 1, 1): (4, 8, 14),    # 588 pixels: two 416-pixel tiles
}
# the split tiles the split rule of make_plan accepts per (split desc, CUS), both passes alike (host arithmetic: blocks < CUS,
# CUS / 2 < blocks * Z <= CUS + CUS / 4, chunks >= 2 * Z); every other (split tile, desc, CUS) combination is declined
SPLIT_ACCEPTS = {
    ((2, 124, 9, 9, 124, 3, 1, 1), 2): {230}, ((2, 124, 9, 9, 124, 3, 1, 1), 4): {231, 233},
    ((2, 124, 9, 9, 124, 3, 1, 1), 8): {232, 234}, ((2, 124, 9, 9, 124, 3, 1, 1), 14): {232, 234, 235},
    ((3, 128, 14, 14, 128, 3, 1, 1), 4): {230, 233}, ((3, 128, 14, 14, 128, 3, 1, 1), 8): {231, 234},
    ((3, 128, 14, 14, 128, 3, 1, 1), 14): {231, 232, 234, 235},
}
# (desc, CUS) in the order the GPU test is parametrised
DESCS = [(d, None) for d in PLAIN_DESCS] + [(d, c) for d, cs in SPLIT_DESCS.items() for c in cs]
# the descs of the import / export contract tests
CONTRACT = (2, 10, 11, 13, 24, 3, 1, 1)   # pinned and unpinned
TWIN = (3, 10, 11, 13, 24, 3, 1, 1)       # "another replica" of it that is never pinned: its launch logs are the rule-based ones
TUNED = (2, 12, 14, 14, 24, 5, 1, 2)      # measured by a real cnn_conv2d_autotune_ws (5x5: the implicit GEMM in both passes)
