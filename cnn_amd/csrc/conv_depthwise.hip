// conv_depthwise.hip -- CNN_CONV2D_DEPTHWISE (one k x k filter per channel): forward, data gradient, weight / bias gradient.
// DESIGN.md 4.1.1.  Nine FMAs per eight bytes moved at 3x3: every pass is HBM-bound, so the kernels are plain VALU code whose
// aim is that each byte of x / dy / y crosses HBM once, in 16-byte accesses per lane where the rows are 16-byte aligned.
//
//   dw_fwd<3x3,s>, dw_dgrad<3x3,s1>  dw3_rows: a lane owns a strip of 4 output columns and walks down a tile of output rows with a rolling
//                                    3-row register window (each input row is loaded once per strip: one float4 + the halo columns,
//                                    which the neighbouring lanes' float4s have already brought into L1).  Work items are numbered
//                                    (plane, row tile, strip) across the whole tensor, so a wave holds as many (b, c) planes as fit --
//                                    32 planes of a 7x7 tensor -- and the 9 weights + bias are per-lane loads (the same address in
//                                    every lane of a large plane: one broadcast request).  The stride-1 data gradient is the same
//                                    kernel with the filter flipped and pad' = 2 - pad.
//   dw_dgrad<3x3,s2>                 dw3_dgrad_s2: gather by output-parity classes -- a dx row reads the one or two dy rows whose taps
//                                    have its parity, a dx column the taps of its parity; no zero insertion.  Rows and columns no
//                                    window covers sum nothing and come out +0.
//   dw_wgrad<3x3,s>                  dw3_wgrad: workgroup (channel, batch slab) walks the slab's planes with the same strips and window;
//                                    a lane keeps 9 tap sums + the dy sum, the wave adds them by shuffles, the workgroup's four waves
//                                    in order, one row [k*k | 1] per (slab, channel) goes to the workspace; reduce_slabs
//                                    (conv_wgrad.hip) adds the slabs and divides: the rounding contract of every other family.
//   dw_*<generic>                    runtime k / s / pad, one output element (or one tap sum) at a time: correct, not fast.
// Padding is zeros in registers, never an out-of-tensor read.  All indices are 32-bit: check_desc refuses tensors of 2^31 elements.
#include "conv_families.h"

// the geometry tag of a specialised launch names the code bodies it chose (the kernel name in front of `|` does not): " off<OFF> v<vst|vdy>"
// (dw3_rows, dw3_wgrad) or " pp<PP> v<vst>" (dw3_dgrad_s2).  tests/depthwise_ref.launch_variants is the same choice on the CPU.
#define DW_TAG(d, key, which, vec) CONV_TAG_FMT " " key "%d v%d", CONV_TAG_ARGS(d), (int)(which), (int)(vec)

namespace cnn_amd {
namespace {

constexpr int kDwBlock = 256;

// rows per tile: whole small planes, else about 8 (the two halo rows are re-read from L2 once per tile).  (Measured, profiles/depthwise.md:
// halving the tiles of the late layers until the launch has four workgroups of items per CU made most of them slower -- the halo
// re-reads cost more than the extra lanes bring.)
inline void dw_tiles(int rows, int* R, int* ntile) {
    *ntile = (rows + 7) / 8;
    *R = (rows + *ntile - 1) / *ntile;
    *ntile = (rows + *R - 1) / *R;
}
inline bool aligned16p(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// v[j] = row[start + j] for j < NW, zero outside the tensor.  OFF >= 0: the rows are 16-byte aligned and start + OFF is a multiple
// of 4, so the columns start + OFF + 4i .. + 3 move as one float4 where they lie inside the row; OFF < 0: scalar loads only.
template <int NW, int OFF>
__device__ __forceinline__ void dw_load_row(const float* __restrict__ plane, int row, int IH, int IW, int start, float (&v)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; ++j) v[j] = 0.f;
    if (row < 0 || row >= IH) return;
    const float* __restrict__ rp = plane + (size_t)row * IW;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const bool in_group = OFF >= 0 && j >= OFF && OFF + (j - OFF) / 4 * 4 + 3 < NW;  // (compile-time after unrolling)
        const bool head = in_group && (j - OFF) % 4 == 0;
        const int col = start + j;
        if (head) {
            if (col >= 0 && col + 3 < IW) {
                const float4 t = *reinterpret_cast<const float4*>(rp + col);
                v[j] = t.x; v[j + 1 < NW ? j + 1 : j] = t.y; v[j + 2 < NW ? j + 2 : j] = t.z; v[j + 3 < NW ? j + 3 : j] = t.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j + u < NW && col + u >= 0 && col + u < IW) v[j + u < NW ? j + u : j] = rp[col + u];
            }
        } else if (!in_group) {
            if (col >= 0 && col < IW) v[j] = rp[col];
        }
    }
}

struct DwRows {
    const float* in;     // [planes][IH][IW]
    const float* w;      // [C][9]
    const float* bias;   // [C], or null (data gradient)
    float* out;          // [planes][OH][OW], nullable in forward mode when out2 is given
    float* out2;         // forward: relu(out), nullable
    const float* below;  // data gradient: output of the ReLU layer below ([planes][OH][OW]), nullable
    int C, IH, IW, OH, OW, pad;
    int R, ntile, nstrip;
    unsigned items;      // planes * ntile * nstrip
    int flip;            // data gradient: the filter rotated by 180 degrees
    int vst;             // the output rows (all given output tensors) are 16-byte aligned and OW % 4 == 0: float4 stores
};

// 3x3 forward (stride S) and the stride-1 data gradient
template <int S, int OFF>
__global__ __launch_bounds__(kDwBlock) void dw3_rows(const DwRows p) {
    const unsigned t = blockIdx.x * (unsigned)kDwBlock + threadIdx.x;
    if (t >= p.items) return;
    const int strip = (int)(t % (unsigned)p.nstrip);
    const unsigned rest = t / (unsigned)p.nstrip;
    const int tile = (int)(rest % (unsigned)p.ntile);
    const unsigned plane = rest / (unsigned)p.ntile;
    const int c = (int)(plane % (unsigned)p.C);
    float wv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wv[i] = p.w[c * 9 + (p.flip ? 8 - i : i)];
    const float bv = p.bias ? p.bias[c] : 0.f;
    const float* __restrict__ ip = p.in + (size_t)plane * p.IH * p.IW;
    const size_t obase = (size_t)plane * p.OH * p.OW;
    constexpr int NW = 3 * S + 3;
    const int q0 = strip * 4, start = q0 * S - p.pad;
    const int p0 = tile * p.R, p1 = p0 + p.R < p.OH ? p0 + p.R : p.OH;
    float r0[NW], r1[NW], r2[NW];
    int row = p0 * S - p.pad;
    dw_load_row<NW, OFF>(ip, row, p.IH, p.IW, start, r0);
    if (S == 1) dw_load_row<NW, OFF>(ip, row + 1, p.IH, p.IW, start, r1);
    for (int pr = p0; pr < p1; ++pr) {
        if (S == 2) dw_load_row<NW, OFF>(ip, row + 1, p.IH, p.IW, start, r1);
        dw_load_row<NW, OFF>(ip, row + 2, p.IH, p.IW, start, r2);
        float acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = bv;
#pragma unroll
            for (int j = 0; j < 3; ++j) a = fmaf(r0[e * S + j], wv[j], a);
#pragma unroll
            for (int j = 0; j < 3; ++j) a = fmaf(r1[e * S + j], wv[3 + j], a);
#pragma unroll
            for (int j = 0; j < 3; ++j) a = fmaf(r2[e * S + j], wv[6 + j], a);
            acc[e] = a;
        }
        const size_t o = obase + (size_t)pr * p.OW + q0;
        if (p.vst) {
            float4 v = make_float4(acc[0], acc[1], acc[2], acc[3]);
            if (p.below) {  // relu.cpp:35-40: dx = (y_below <= 0) ? 0 : dx
                const float4 m = *reinterpret_cast<const float4*>(p.below + o);
                v.x = m.x <= 0.f ? 0.f : v.x; v.y = m.y <= 0.f ? 0.f : v.y; v.z = m.z <= 0.f ? 0.f : v.z; v.w = m.w <= 0.f ? 0.f : v.w;
            }
            if (p.out) *reinterpret_cast<float4*>(p.out + o) = v;
            if (p.out2)  // relu.cpp:21-26: y >= 0 ? y : 0
                *reinterpret_cast<float4*>(p.out2 + o) =
                    make_float4(v.x >= 0.f ? v.x : 0.f, v.y >= 0.f ? v.y : 0.f, v.z >= 0.f ? v.z : 0.f, v.w >= 0.f ? v.w : 0.f);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (q0 + e >= p.OW) continue;
                float v = acc[e];
                if (p.below) v = p.below[o + e] <= 0.f ? 0.f : v;
                if (p.out) p.out[o + e] = v;
                if (p.out2) p.out2[o + e] = v >= 0.f ? v : 0.f;
            }
        }
        if (S == 1) {
#pragma unroll
            for (int j = 0; j < NW; ++j) { r0[j] = r1[j]; r1[j] = r2[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < NW; ++j) r0[j] = r2[j];
        }
        row += S;
    }
}

struct DwS2 {
    const float* dy;     // [planes][Ho][Wo]
    const float* w;      // [C][9]
    float* dx;           // [planes][H][W]
    const float* below;  // nullable, [planes][H][W]
    int C, H, W, Ho, Wo, pad;
    int R, ntile, nstrip;
    unsigned items;
    int vst;
};

// 3x3 stride-2 data gradient.  dx[h][w] = sum over (i, j) with (h + pad - i), (w + pad - j) even of dy[(h + pad - i) / 2][(w + pad - j) / 2] * w[i][j].
// PP = pad & 1: with the strip's first column a multiple of 4 the parity of every column, and which of the 4 loaded dy columns a tap
// reads, are compile-time.
template <int PP>
__global__ __launch_bounds__(kDwBlock) void dw3_dgrad_s2(const DwS2 p) {
    const unsigned t = blockIdx.x * (unsigned)kDwBlock + threadIdx.x;
    if (t >= p.items) return;
    const int strip = (int)(t % (unsigned)p.nstrip);
    const unsigned rest = t / (unsigned)p.nstrip;
    const int tile = (int)(rest % (unsigned)p.ntile);
    const unsigned plane = rest / (unsigned)p.ntile;
    const int c = (int)(plane % (unsigned)p.C);
    float wv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wv[i] = p.w[c * 9 + i];
    const float* __restrict__ dyp = p.dy + (size_t)plane * p.Ho * p.Wo;
    const size_t obase = (size_t)plane * p.H * p.W;
    const int w0 = strip * 4;
    const int qlo = w0 / 2 + (p.pad - PP) / 2 - 1;  // the dy columns qlo .. qlo + 3 hold every tap of the four dx columns
    const int h0 = tile * p.R, h1 = h0 + p.R < p.H ? h0 + p.R : p.H;
    for (int h = h0; h < h1; ++h) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const int hp = h + p.pad;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if ((hp - i) & 1) continue;
            const int pr = (hp - i) >> 1;
            if (pr < 0 || pr >= p.Ho) continue;
            const float* __restrict__ rp = dyp + (size_t)pr * p.Wo;
            float dq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) dq[u] = (qlo + u >= 0 && qlo + u < p.Wo) ? rp[qlo + u] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (((PP + e - j) & 1) == 0) acc[e] = fmaf(dq[(PP + e - j) / 2 + 1], wv[i * 3 + j], acc[e]);
        }
        const size_t o = obase + (size_t)h * p.W + w0;
        if (p.vst) {
            float4 v = make_float4(acc[0], acc[1], acc[2], acc[3]);
            if (p.below) {
                const float4 m = *reinterpret_cast<const float4*>(p.below + o);
                v.x = m.x <= 0.f ? 0.f : v.x; v.y = m.y <= 0.f ? 0.f : v.y; v.z = m.z <= 0.f ? 0.f : v.z; v.w = m.w <= 0.f ? 0.f : v.w;
            }
            *reinterpret_cast<float4*>(p.dx + o) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (w0 + e >= p.W) continue;
                float v = acc[e];
                if (p.below) v = p.below[o + e] <= 0.f ? 0.f : v;
                p.dx[o + e] = v;
            }
        }
    }
}

// ---- generic: runtime k / s / pad, one output element per thread ----
struct DwAny {
    const float* in;
    const float* w;      // [C][k*k]
    const float* bias;
    float* out;
    float* out2;
    const float* below;
    int C, H, W, Ho, Wo, k, s, pad;  // H x W: x / dx, Ho x Wo: y / dy
    unsigned n;          // output elements
};

__global__ __launch_bounds__(kDwBlock) void dw_any_fwd(const DwAny p) {
    const unsigned t = blockIdx.x * (unsigned)kDwBlock + threadIdx.x;
    if (t >= p.n) return;
    const int q = (int)(t % (unsigned)p.Wo);
    const unsigned rest = t / (unsigned)p.Wo;
    const int pr = (int)(rest % (unsigned)p.Ho);
    const unsigned plane = rest / (unsigned)p.Ho;
    const int c = (int)(plane % (unsigned)p.C);
    const float* __restrict__ ip = p.in + (size_t)plane * p.H * p.W;
    const float* __restrict__ wp = p.w + (size_t)c * p.k * p.k;
    float a = p.bias[c];
    for (int i = 0; i < p.k; ++i) {
        const int r = pr * p.s - p.pad + i;
        if (r < 0 || r >= p.H) continue;
        for (int j = 0; j < p.k; ++j) {
            const int col = q * p.s - p.pad + j;
            if (col < 0 || col >= p.W) continue;
            a = fmaf(ip[(size_t)r * p.W + col], wp[i * p.k + j], a);
        }
    }
    if (p.out) p.out[t] = a;
    if (p.out2) p.out2[t] = a >= 0.f ? a : 0.f;
}

__global__ __launch_bounds__(kDwBlock) void dw_any_dgrad(const DwAny p) {
    const unsigned t = blockIdx.x * (unsigned)kDwBlock + threadIdx.x;
    if (t >= p.n) return;
    const int wc = (int)(t % (unsigned)p.W);
    const unsigned rest = t / (unsigned)p.W;
    const int h = (int)(rest % (unsigned)p.H);
    const unsigned plane = rest / (unsigned)p.H;
    const int c = (int)(plane % (unsigned)p.C);
    const float* __restrict__ dyp = p.in + (size_t)plane * p.Ho * p.Wo;
    const float* __restrict__ wp = p.w + (size_t)c * p.k * p.k;
    float a = 0.f;
    for (int i = 0; i < p.k; ++i) {
        const int hp = h + p.pad - i;
        if (hp < 0 || hp % p.s != 0) continue;
        const int pr = hp / p.s;
        if (pr >= p.Ho) continue;
        for (int j = 0; j < p.k; ++j) {
            const int wq = wc + p.pad - j;
            if (wq < 0 || wq % p.s != 0) continue;
            const int q = wq / p.s;
            if (q >= p.Wo) continue;
            a = fmaf(dyp[(size_t)pr * p.Wo + q], wp[i * p.k + j], a);
        }
    }
    if (p.below) a = p.below[t] <= 0.f ? 0.f : a;
    p.out[t] = a;
}

// ---- weight / bias gradient ----
struct DwWgrad {
    const float* x;   // [B][C][H][W]
    const float* dy;  // [B][C][Ho][Wo]
    float* slabs;     // [slots][C][k*k + 1]
    int B, C, H, W, Ho, Wo, k, s, pad;
    int per;          // samples per slab
    int R, ntile, nstrip;
    int vdy;          // the dy rows are 16-byte aligned and Wo % 4 == 0
};

// adds v over the workgroup in a fixed order (shuffle tree per wave, then the waves in order); the sum is valid in thread 0
__device__ __forceinline__ float dw_block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // (red is reused from call to call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float tsum = 0.f;
    if (threadIdx.x == 0)
        for (int k = 0; k < kDwBlock / 64; ++k) tsum += red[k];
    return tsum;
}

template <int S, int OFF>
__global__ __launch_bounds__(kDwBlock) void dw3_wgrad(const DwWgrad p) {
    __shared__ float red[kDwBlock / 64];
    const int c = blockIdx.x, slot = blockIdx.y;
    const int b0 = slot * p.per, b1 = b0 + p.per < p.B ? b0 + p.per : p.B;
    constexpr int NW = 3 * S + 3;
    float acc[9], accb = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.f;
    const int per_plane = p.ntile * p.nstrip, items = (b1 - b0) * per_plane;
    for (int it = threadIdx.x; it < items; it += kDwBlock) {
        const int strip = it % p.nstrip, rest = it / p.nstrip;
        const int tile = rest % p.ntile, b = b0 + rest / p.ntile;
        const size_t plane = (size_t)b * p.C + c;
        const float* __restrict__ xp = p.x + plane * p.H * p.W;
        const float* __restrict__ dyp = p.dy + plane * p.Ho * p.Wo;
        const int q0 = strip * 4, start = q0 * S - p.pad;
        const int p0 = tile * p.R, p1 = p0 + p.R < p.Ho ? p0 + p.R : p.Ho;
        float r0[NW], r1[NW], r2[NW];
        int row = p0 * S - p.pad;
        dw_load_row<NW, OFF>(xp, row, p.H, p.W, start, r0);
        if (S == 1) dw_load_row<NW, OFF>(xp, row + 1, p.H, p.W, start, r1);
        for (int pr = p0; pr < p1; ++pr) {
            if (S == 2) dw_load_row<NW, OFF>(xp, row + 1, p.H, p.W, start, r1);
            dw_load_row<NW, OFF>(xp, row + 2, p.H, p.W, start, r2);
            const float* __restrict__ dr = dyp + (size_t)pr * p.Wo + q0;
            float dv[4] = {0.f, 0.f, 0.f, 0.f};
            if (p.vdy) {
                const float4 v = *reinterpret_cast<const float4*>(dr);
                dv[0] = v.x; dv[1] = v.y; dv[2] = v.z; dv[3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (q0 + e < p.Wo) dv[e] = dr[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (q0 + e >= p.Wo) continue;  // (a column that does not exist adds nothing, whatever x holds there)
                accb += dv[e];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    acc[j] = fmaf(dv[e], r0[e * S + j], acc[j]);
                    acc[3 + j] = fmaf(dv[e], r1[e * S + j], acc[3 + j]);
                    acc[6 + j] = fmaf(dv[e], r2[e * S + j], acc[6 + j]);
                }
            }
            if (S == 1) {
#pragma unroll
                for (int j = 0; j < NW; ++j) { r0[j] = r1[j]; r1[j] = r2[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < NW; ++j) r0[j] = r2[j];
            }
            row += S;
        }
    }
    float* out = p.slabs + ((size_t)slot * p.C + c) * 10;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float v = dw_block_sum(acc[i], red);
        if (threadIdx.x == 0) out[i] = v;
    }
    const float vb = dw_block_sum(accb, red);
    if (threadIdx.x == 0) out[9] = vb;
}

// one tap sum (or the dy sum) at a time over the slab's pixels
__global__ __launch_bounds__(kDwBlock) void dw_any_wgrad(const DwWgrad p) {
    __shared__ float red[kDwBlock / 64];
    const int c = blockIdx.x, slot = blockIdx.y;
    const int b0 = slot * p.per, b1 = b0 + p.per < p.B ? b0 + p.per : p.B;
    const int kk = p.k * p.k, P = p.Ho * p.Wo;
    float* out = p.slabs + ((size_t)slot * p.C + c) * (kk + 1);
    for (int tap = 0; tap <= kk; ++tap) {
        const int i = tap / p.k, j = tap % p.k;
        float a = 0.f;
        for (int b = b0; b < b1; ++b) {
            const size_t plane = (size_t)b * p.C + c;
            const float* __restrict__ xp = p.x + plane * p.H * p.W;
            const float* __restrict__ dyp = p.dy + plane * P;
            for (int pix = threadIdx.x; pix < P; pix += kDwBlock) {
                const float dv = dyp[pix];
                if (tap == kk) {
                    a += dv;
                    continue;
                }
                const int r = pix / p.Wo * p.s - p.pad + i, col = pix % p.Wo * p.s - p.pad + j;
                if (r < 0 || r >= p.H || col < 0 || col >= p.W) continue;
                a = fmaf(dv, xp[(size_t)r * p.W + col], a);
            }
        }
        const float v = dw_block_sum(a, red);
        if (threadIdx.x == 0) out[tap] = v;
    }
}

// CNN_AMD_DW_GENERIC=1: every geometry through the generic kernels (A/B measurements; both sides are correct kernels)
bool dw_specialised(const cnn_conv2d_desc* d) { return d->k == 3 && (d->s == 1 || d->s == 2) && CNN_OPT_INT("DW_GENERIC", 0) == 0; }

// OFF of dw_load_row for rows of `IW` floats at `base`, window start = 4 * strip * S - pad
int dw_off(const float* base, int IW, int pad) {
    if (!aligned16p(base) || IW % 4 != 0) return -1;
    const int off = ((pad % 4) + 4) % 4;
    return off <= 2 ? off : -1;
}

template <int S>
int launch_rows(const cnn_conv2d_desc* d, const char* name, const DwRows& p, int off, hipStream_t s) {
    const unsigned grid = (p.items + kDwBlock - 1) / kDwBlock;
    switch (off) {
        case 0: CNN_KLAUNCH(s, name, (dw3_rows<S, 0><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vst)); break;
        case 1: CNN_KLAUNCH(s, name, (dw3_rows<S, 1><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vst)); break;
        case 2: CNN_KLAUNCH(s, name, (dw3_rows<S, 2><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vst)); break;
        default: CNN_KLAUNCH(s, name, (dw3_rows<S, -1><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vst)); break;
    }
    return CNN_AMD_OK;
}

template <int S>
int launch_wgrad3(const cnn_conv2d_desc* d, const char* name, const DwWgrad& p, int off, dim3 grid, hipStream_t s) {
    switch (off) {
        case 0: CNN_KLAUNCH(s, name, (dw3_wgrad<S, 0><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vdy)); break;
        case 1: CNN_KLAUNCH(s, name, (dw3_wgrad<S, 1><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vdy)); break;
        case 2: CNN_KLAUNCH(s, name, (dw3_wgrad<S, 2><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vdy)); break;
        default: CNN_KLAUNCH(s, name, (dw3_wgrad<S, -1><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "off", off, p.vdy)); break;
    }
    return CNN_AMD_OK;
}

// samples per batch slab: about four workgroups per CU over the C channels, at least one sample, at most the batch
int dw_slab_samples(const cnn_conv2d_desc* d) {
    long long want = ((long long)4 * num_cus() + d->Ci - 1) / d->Ci;
    if (want < 1) want = 1;
    if (want > d->B) want = d->B;
    return (int)((d->B + want - 1) / want);
}

}  // namespace

int dw_run(const cnn_conv2d_desc* d, int mode, const float* in, const float* w, const float* bias, float* out, float* out2, hipStream_t s) {
    const int Ho = cnn_conv2d_out_dim(d->H, d->k, d->s, d->pad), Wo = cnn_conv2d_out_dim(d->W, d->k, d->s, d->pad);
    const unsigned planes = (unsigned)d->B * (unsigned)d->Ci;
    const bool fwd = mode == MODE_FWD;
    // the tensor the pass reads / writes
    const int IH = fwd ? d->H : Ho, IW = fwd ? d->W : Wo, OH = fwd ? Ho : d->H, OW = fwd ? Wo : d->W;
    const bool vst = OW % 4 == 0 && (!out || aligned16p(out)) && (!out2 || aligned16p(out2));
    if (dw_specialised(d) && (fwd || d->s == 1)) {
        DwRows p;
        p.in = in; p.w = w; p.bias = fwd ? bias : nullptr;
        p.out = out; p.out2 = fwd ? out2 : nullptr; p.below = fwd ? nullptr : out2;
        p.C = d->Ci; p.IH = IH; p.IW = IW; p.OH = OH; p.OW = OW;
        p.pad = fwd ? d->pad : 2 - d->pad;
        p.nstrip = (OW + 3) / 4;
        dw_tiles(OH, &p.R, &p.ntile);
        p.items = planes * (unsigned)p.ntile * (unsigned)p.nstrip;
        p.flip = fwd ? 0 : 1;
        p.vst = vst ? 1 : 0;
        const int off = dw_off(in, IW, p.pad);
        if (fwd) return d->s == 1 ? launch_rows<1>(d, "dw_fwd<3x3,s1>", p, off, s) : launch_rows<2>(d, "dw_fwd<3x3,s2>", p, off, s);
        return launch_rows<1>(d, "dw_dgrad<3x3,s1>", p, off, s);
    }
    if (dw_specialised(d)) {  // the stride-2 data gradient
        DwS2 p;
        p.dy = in; p.w = w; p.dx = out; p.below = out2;
        p.C = d->Ci; p.H = d->H; p.W = d->W; p.Ho = Ho; p.Wo = Wo; p.pad = d->pad;
        p.nstrip = (d->W + 3) / 4;
        dw_tiles(d->H, &p.R, &p.ntile);
        p.items = planes * (unsigned)p.ntile * (unsigned)p.nstrip;
        p.vst = vst ? 1 : 0;
        const unsigned grid = (p.items + kDwBlock - 1) / kDwBlock;
        if (d->pad & 1) CNN_KLAUNCH(s, "dw_dgrad<3x3,s2>", (dw3_dgrad_s2<1><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "pp", 1, p.vst));
        else CNN_KLAUNCH(s, "dw_dgrad<3x3,s2>", (dw3_dgrad_s2<0><<<grid, kDwBlock, 0, s>>>(p)), DW_TAG(d, "pp", 0, p.vst));
        return CNN_AMD_OK;
    }
    DwAny p;
    p.in = in; p.w = w; p.bias = bias; p.out = out; p.out2 = fwd ? out2 : nullptr; p.below = fwd ? nullptr : out2;
    p.C = d->Ci; p.H = d->H; p.W = d->W; p.Ho = Ho; p.Wo = Wo; p.k = d->k; p.s = d->s; p.pad = d->pad;
    p.n = planes * (unsigned)OH * (unsigned)OW;
    const unsigned grid = (p.n + kDwBlock - 1) / kDwBlock;
    if (fwd) CNN_KLAUNCH(s, "dw_fwd<generic>", (dw_any_fwd<<<grid, kDwBlock, 0, s>>>(p)), CONV_TAG(d));
    else CNN_KLAUNCH(s, "dw_dgrad<generic>", (dw_any_dgrad<<<grid, kDwBlock, 0, s>>>(p)), CONV_TAG(d));
    return CNN_AMD_OK;
}

int dw_wgrad_slots(const cnn_conv2d_desc* d) {
    const int per = dw_slab_samples(d);
    return (d->B + per - 1) / per;
}

int dw_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s) {
    DwWgrad p;
    p.x = x; p.dy = dy; p.slabs = slabs;
    p.B = d->B; p.C = d->Ci; p.H = d->H; p.W = d->W; p.k = d->k; p.s = d->s; p.pad = d->pad;
    p.Ho = cnn_conv2d_out_dim(d->H, d->k, d->s, d->pad);
    p.Wo = cnn_conv2d_out_dim(d->W, d->k, d->s, d->pad);
    p.per = dw_slab_samples(d);
    p.nstrip = (p.Wo + 3) / 4;
    dw_tiles(p.Ho, &p.R, &p.ntile);
    p.vdy = (p.Wo % 4 == 0 && aligned16p(dy)) ? 1 : 0;
    const dim3 grid((unsigned)d->Ci, (unsigned)((d->B + p.per - 1) / p.per));
    CNN_REQUIRE(grid.y <= 65535u, "cnn_conv2d_backward_weight: %u depthwise batch slabs", grid.y);
    if (dw_specialised(d)) {
        const int off = dw_off(x, d->W, d->pad);
        return d->s == 1 ? launch_wgrad3<1>(d, "dw_wgrad<3x3,s1>", p, off, grid, s) : launch_wgrad3<2>(d, "dw_wgrad<3x3,s2>", p, off, grid, s);
    }
    CNN_KLAUNCH(s, "dw_wgrad<generic>", (dw_any_wgrad<<<grid, kDwBlock, 0, s>>>(p)), CONV_TAG(d));
    return CNN_AMD_OK;
}

}  // namespace cnn_amd
