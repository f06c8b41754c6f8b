// lds_dma.h -- buffer-addressed LDS DMA, shared by every kernel that stages operands with it (the row kernels: rows_common.h; the
// LDS-staged weight gradients: wgrad_sp_common.h).
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_void_ptr;

// one LDS-DMA instruction through a buffer descriptor: lane l moves 16 bytes from base + voff(l) + soff to lds + l*4 floats.  A lane whose
// voff lies outside the buffer moves ZEROS (probed on MI355X: tools/probes/buflds_probe.cpp) -- that is how pad floats, channels
// behind the tensor, halo rows outside the image and the missing second sample of an odd batch are staged: every instruction runs
// with all 64 lanes and no branch around it.  kOob is such an offset for every descriptor (byte sizes stay below 2^31).
constexpr unsigned kOob = 0x80000000u;
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, float* lds) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_ptr)lds, 16, (int)voff, (int)soff, 0, 0);
}

}  // namespace
