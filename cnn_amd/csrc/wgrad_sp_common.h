// wgrad_sp_common.h -- what the LDS-staged output-stationary weight gradients share: conv_wgrad_sp.hip (3x3 /
// stride 1, the BASELINE plane widths), conv_wgrad_sp2.hip (stride 2) and conv_wgrad_sp_any.hip (stride 1, any plane size).  A sibling
// owns its parameter struct (with the fields x, dy, slabs, Ci, Co, Ntot, pitch, stages_total, stages_per_block), its geometry struct
// (BUF, OP, lds_bytes, ...), its planner and its kernel body: the LDS zero fill, the stage loop with its dma_slot / read_ops / seg_mfma
// lambdas and the slab epilogue.  The zero fill, the accumulator zeroing and the epilogue are the same text in all three kernels and
// stay there: as inlined functions each of them changed the register allocation of the whole kernel, the tuned stage loop included
// (profiles/wgrad_sp_family.md).  What is here compiles to the same machine code as the copies it replaced: change a device piece
// only together with a comparison of the three files' assembly against the commit before.
#pragma once
#include <cstdlib>

#include "conv_families.h"
#include "lds_dma.h"

using namespace cnn_amd;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 64;  // output channels per workgroup tile

// plane strides for 16-byte DMA units: a multiple of 4 floats with an odd number of 16-byte pieces (4-way bank conflicts at most)
constexpr int stride_for(int len) { return (((len + 3) / 4) & 1) ? (len + 3) / 4 * 4 : (len + 3) / 4 * 4 + 4; }

// the stages [s_lo, s_hi) of workgroup blockIdx.x
template <class P>
__device__ __forceinline__ void sp_stage_range(const P& p, int* s_lo, int* s_hi) {
    *s_lo = blockIdx.x * p.stages_per_block;
    *s_hi = *s_lo + p.stages_per_block < p.stages_total ? *s_lo + p.stages_per_block : p.stages_total;
}

// ---- host side
// (buffer descriptors: byte sizes below 2^31) x is [B][Ci][H][W], dy [B][Co][ho][wo]
inline bool sp_descriptors_fit(const cnn_conv2d_desc* d, int ho, int wo) {
    return (long long)d->B * d->Ci * d->H * d->W < (1ll << 29) && (long long)d->B * d->Co * ho * wo < (1ll << 29);
}

// the stages of a (gy x gz)-tile grid over the chip: one workgroup per CU (LDS), or SP_BLOCKS workgroups in all
inline void sp_partition(int stages_total, int gy, int gz, int* stages_per_block, int* kblocks) {
    const int env = CNN_OPT_INT("SP_BLOCKS", 0);
    split_units(stages_total, (env > 0 ? env : num_cus()) / ((long long)gy * gz), stages_per_block, kblocks);
}

// launch one instance: Geom = its geometry (one attribute flag per instance), pl = its plan {p, kblocks, gy, gz}, `name` its launch-log name
template <class Geom, class Plan, class P>
int sp_launch(void (*kern)(const P), const char* name, const Plan& pl, const cnn_conv2d_desc* d, int pad, hipStream_t s) {
    static DeviceOnce attr_once;
    if (int rc = allow_dynamic_lds(attr_once, (int)Geom::lds_bytes, kern)) return rc;
    const dim3 grid(pl.kblocks, pl.gy, pl.gz);
    CNN_KLAUNCH(s, name, (kern<<<grid, 256, Geom::lds_bytes, s>>>(pl.p)), "B%d Ci%d %dx%d Co%d k3 s%d p%d slabs%d", d->B, d->Ci, d->H, d->W, d->Co, d->s, pad,
                pl.kblocks);
    return CNN_AMD_OK;
}

}  // namespace
