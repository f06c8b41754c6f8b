// augment.hip -- geometric augmentation of uint8 image batches on the device (an addition: the reference's ImageAugmentor runs OpenCV on
// the host, pipeline.cpp:40-77): flip, crop, rotate and the resize to the network's size as ONE per-sample affine gather, fused with the
// bytes -> fp32 planar conversion the u8 stager does anyway (staging.hip, u8hwc_to_f32chw).  Decode stays on the host.
//
// The rule (restated in NumPy by tests/augment_ref.py; the kernel equals it bit for bit).  Input: interleaved bytes [B][Hs][Ws][3];
// output: planar fp32 [B][3][H][W]; sample b has six floats m[b][0..5] that map OUTPUT pixel indices to SOURCE pixel indices.  Per output
// pixel (x, y), all in fp32, every product and sum rounded separately:
//     sx = (m0*x + m1*y) + m2            sy = (m3*x + m4*y) + m5
//     inside = sx >= -0.5f && sx <= Ws-0.5f && sy >= -0.5f && sy <= Hs-0.5f
//     x0f = floorf(sx); fx = sx - x0f;   y0f = floorf(sy); fy = sy - y0f
//     x0 = clamp((int)x0f, 0, Ws-1); x1 = clamp((int)x0f + 1, 0, Ws-1)      (same for y)
//     t.. = lut[byte]                    (the stager's table: v * 1.f / 255 computed on the host)
//     top = t00 + fx*(t01 - t00); bot = t10 + fx*(t11 - t10); out = top + fy*(bot - top)
//     out = inside ? out : fill
// A position inside the source's pixel area reads edge-replicated taps (what a resize needs), a position outside it gives `fill` (a
// rotation's corners: the constant border).  With fx == 0 the rule yields t00 exactly, so the identity, flips, integer shifts and
// quarter turns are bit-identical to the plain conversion of the permuted image.  Two taps per axis whatever the scale: a shrink ratio of
// 2 or more aliases, except out of a dataset with half-size levels (below).
//
// The photometric epilogue (the kPhoto instantiations, reached through a photo stager only: cnn_batch_stager_create_u8_photo; restated in
// NumPy by tests/photo_ref.py, bit for bit as well).  Sample b has 20 floats p[b][0..19], the stager has s[3], t[3] and a clamp flag.  Per
// output pixel, behind the rule above, every product and sum rounded separately:
//     v0,v1,v2 = the gather rule's three channel values of this pixel (inside pixels only)
//     u_c   = ((A[c][0]*v0 + A[c][1]*v1) + A[c][2]*v2) + o[c]        A = p[0..8] row-major, o = p[9..11]
//     u_c   = clamp ? fminf(fmaxf(u_c, 0), 1) : u_c
//     out_c = u_c * s[c] + t[c]                                      (normalisation: s = 1/std, t = -mean/std)
//     out_c = inside ? out_c : fill                                  (fill is in OUTPUT units: the colour stage does not touch it)
//     ex0,ey0,ew,eh = p[12..15] (whole numbers), ev[c] = p[16..18], p[19] reserved = 0
//     out_c = (ex0 <= x && x < ex0+ew && ey0 <= y && y < ey0+eh) ? ev[c] : out_c     (fp32 comparisons; ev in output units)
// ew == 0 or eh == 0 is no box.  With A = I, o = 0, clamp off, s = 1, t = 0 and no box the epilogue returns the gather rule's bits: the
// table holds finite values >= 0, so 1*v + 0*w == v, v + 0 == v and v*1 + 0 == v.  The parameters are pinned memory the caller writes
// and are not checked: a non-finite one gives unspecified PIXELS, never an access out of bounds -- the box only selects between two
// values per pixel (a NaN bound compares false: no box), it never forms an address.
//
// The resident stager's kernel (the kResident instantiations, reached through cnn_batch_stager_create_u8_resident only; restated by
// tests/resident_ref.py): the same two rules with sample b's source taken from a dataset's store, idx = indices[b]:
//     source = store + (size_t)idx * (Hs*Ws*3);   idx == -1: no pixel of the sample is inside, no byte of the store is read
//     labels_out[b] = idx < 0 ? -1 : labels[idx]
//
// Half-size levels (the kLevels instantiations, reached through a resident stager on a dataset with more than one level only; restated by
// tests/mip_ref.py; the contract is in include/cnn_amd.h).  Level l > 0 of an image is the edge-replicated 2 x 2 box of level l - 1,
// rounded half up, in integers (dataset_halve_u8 below, at write time).  The host picks a level per sample from the map's scale and
// rewrites the map for that level (cnn_augment_level); the kernel applies the rules above to image idx of level l with Hs, Ws := H_l, W_l:
//     source = store + base[l] + (size_t)idx * (H_l*W_l*3)
#include <cmath>
#include <cstring>
#include <mutex>

#include "common.h"

using namespace cnn_amd;

namespace {

constexpr int kBlock = 256;  // (kMaxDim, kMaxLevels: stager_layout.h)

// where output pixel (x, y) samples the source: the byte offsets of the four taps inside the sample's image and the two weights
struct Taps {
    bool inside;
    int o00, o01, o10, o11;
    float fx, fy;
};
__device__ __forceinline__ Taps augment_taps(float m0, float m1, float m2, float m3, float m4, float m5, int x, int y, int Hs, int Ws) {
#pragma clang fp contract(off)
    const float xf = (float)x, yf = (float)y;
    const float ax = m0 * xf, bx = m1 * yf, ay = m3 * xf, by = m4 * yf;
    const float sx = (ax + bx) + m2;
    const float sy = (ay + by) + m5;
    Taps t;
    t.inside = sx >= -0.5f && sx <= (float)Ws - 0.5f && sy >= -0.5f && sy <= (float)Hs - 0.5f;  // (false for a NaN)
    const float x0f = floorf(sx), y0f = floorf(sy);
    t.fx = sx - x0f;
    t.fy = sy - y0f;
    const int xi = t.inside ? (int)x0f : 0, yi = t.inside ? (int)y0f : 0;  // inside: -1 .. Ws-1 / Hs-1
    const int x0 = min(max(xi, 0), Ws - 1), x1 = min(max(xi + 1, 0), Ws - 1);
    const int y0 = min(max(yi, 0), Hs - 1), y1 = min(max(yi + 1, 0), Hs - 1);
    t.o00 = (y0 * Ws + x0) * 3;
    t.o01 = (y0 * Ws + x1) * 3;
    t.o10 = (y1 * Ws + x0) * 3;
    t.o11 = (y1 * Ws + x1) * 3;
    return t;
}
// the blend of the rule.  With fx == 0 and fy == 0 it is t00 exactly (the table holds finite non-negative values: t00 + 0 * d == t00)
__device__ __forceinline__ float augment_blend(float t00, float t01, float t10, float t11, float fx, float fy) {
#pragma clang fp contract(off)
    const float dt = t01 - t00, db = t11 - t10;
    const float pt = fx * dt, pb = fx * db;
    const float top = t00 + pt, bot = t10 + pb;
    const float dv = bot - top;
    const float pv = fy * dv;
    return top + pv;
}

// the photometric epilogue of one channel: the colour row, the clamp and the normalisation
__device__ __forceinline__ float photo_channel(float a0, float a1, float a2, float o, float v0, float v1, float v2, bool clamp, float s, float t) {
#pragma clang fp contract(off)
    const float p0 = a0 * v0, p1 = a1 * v1, p2 = a2 * v2;
    const float s01 = p0 + p1;
    const float s012 = s01 + p2;
    float u = s012 + o;
    u = clamp ? fminf(fmaxf(u, 0.f), 1.f) : u;
    const float n = u * s;
    return n + t;
}

// the bytes of two neighbours in a row in one load at any byte address (a wave's lanes are 12 source bytes apart at best, so a load
// instruction touches many cache lines whatever its width: the number of loads, not their bytes, is what the four-tap gather pays for)
__device__ __forceinline__ unsigned long long load_u64(const unsigned char* p) {
    unsigned long long w;
    __builtin_memcpy(&w, p, 8);
    return w;
}

// A thread owns four consecutive output pixels of one row of one sample (blockIdx.y: the six matrix floats are uniform loads); kQuad
// (W % 4 == 0, dst 16-byte aligned): one 16-byte store into each channel plane; otherwise per-pixel stores behind a bound on x.  The
// table lives in LDS, as in u8hwc_to_f32chw.  Three routes per thread, the same bits on each: no pixel of the four inside the source --
// no loads; every inside pixel on a whole source pixel (identity, flips, integer shifts, quarter turns) -- one tap each, byte loads;
// otherwise four taps each: taps 00 and 01 are the same pixel or neighbours in a row, so an 8-byte load per source row holds both.  A
// load that would end behind the sample starts early enough to end with it (the pixel's bytes are then shifted down: a tap begins at
// most 5 bytes into its load).  No branch between the loads (an outside pixel's taps are clamped to pixel 0 and not used): they are
// all in flight together.  Offsets inside one sample fit an int (8192 * 8192 * 3), the sample bases are 64-bit.
// kPhoto: the photometric epilogue on the twelve values right before the store.  The sample's 20 floats are uniform loads like the matrix
// (`photo` is [B][20]); the stager's six and the clamp flag arrive as kernel arguments.  A pixel in the erase box counts as not inside
// for the loads (a quad wholly in the box takes the no-load route) and gets ev[c] by a per-element select, so a box edge may cut a quad.
// kResident (the resident stager's kernel, augment_u8_resident): `src` is a dataset's image store and sample b's source is sample
// idx = indices[b] of it, a uniform load like the matrix; the sample base is formed in 64 bits (the store may exceed 4 GiB) before any
// offset inside the sample is added, and the pulled-back load above stays bounded by the SAMPLE (one that ran past sample idx would read
// sample idx + 1, or leave the allocation behind the last one).  idx == -1: no pixel of the sample is inside, so every thread takes the
// no-load route and no byte of the store is read; fill and the erase box apply as ever.  The stager has checked the indices on the host;
// one that is not in [0, N) here is treated as -1 all the same, so that no index can form an address outside the store.  One lane of one
// workgroup per sample writes labels_out[b] = idx < 0 ? -1 : labels[idx].  (PhotoNorm, ResidentArgs: common.h)
// kLevels (augment_u8_resident_levels): `mats` holds the LEVEL maps and sample b reads image idx of level l = levels[b], two more uniform
// loads: the level, and that level's row of the dataset's table -- Hs, Ws, the sample's byte count and the level's base.  sample_bytes,
// `wide` and the pulled-back load's bound are then the LEVEL's sample's (a load that ran past a level-l sample would read its neighbour,
// or leave the allocation behind the last sample of the last level; a level of one or two pixels takes the byte-load route).  A level
// that is not in [0, L) is treated as 0; the taps are clamped to the level's own size whatever the map says, so no value can form an
// address outside the store.
template <bool kQuad, bool kPhoto, bool kResident = false, bool kLevels = false>
__global__ __launch_bounds__(kBlock) void augment_u8_kernel(const unsigned char* __restrict__ src, const float* __restrict__ mats,
                                                            const float* __restrict__ lut_g, float* __restrict__ dst, int Hs0, int Ws0, int H,
                                                            int W, int W4, float fill, const float* __restrict__ photo, PhotoNorm norm,
                                                            ResidentArgs res) {
    __shared__ float lut[256];
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
    const size_t b = blockIdx.y;
    const float* m = mats + 6 * b;
    const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    int Hs = Hs0, Ws = Ws0, sample_bytes = Hs0 * Ws0 * 3;
    if (kLevels) {
        const int l = res.levels[b];
        const DatasetLevel lv = res.table[(l >= 0 && l < res.L) ? l : 0];
        Hs = lv.H;
        Ws = lv.W;
        sample_bytes = lv.sample_bytes;
        src += lv.base;
    }
    float pp[20];
    if (kPhoto) {
#pragma unroll
        for (int k = 0; k < 20; ++k) pp[k] = photo[20 * b + k];
    }
    const float ex1 = kPhoto ? pp[12] + pp[14] : 0.f, ey1 = kPhoto ? pp[13] + pp[15] : 0.f;
    long long idx = (long long)b;  // which sample of `src` this one reads
    if (kResident) {
        const int i = res.indices[b];
        idx = (i >= 0 && (long long)i < res.N) ? (long long)i : -1;
        if (blockIdx.x == 0 && threadIdx.x == 0) res.labels_out[b] = idx < 0 ? -1 : res.labels[idx];
    }
    const bool present = !kResident || idx >= 0;
    const unsigned char* s = src + (size_t)(present ? idx : 0) * (size_t)sample_bytes;
    const size_t plane = (size_t)H * W;
    float* d = dst + b * 3 * plane;
    const int quads = H * W4;
    const bool wide = sample_bytes >= 8;
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < quads; q += gridDim.x * kBlock) {
        const int y = q / W4, x = (q - y * W4) * 4;
        Taps t[4];
        bool box[4] = {false, false, false, false};
        bool any = false, whole = true;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            t[i] = augment_taps(m0, m1, m2, m3, m4, m5, x + i, y, Hs, Ws);
            t[i].inside = t[i].inside && (kQuad || x + i < W) && present;
            if (kPhoto) {
                const float xf = (float)(x + i), yf = (float)y;
                box[i] = xf >= pp[12] && xf < ex1 && yf >= pp[13] && yf < ey1;
                t[i].inside = t[i].inside && !box[i];
            }
            any = any || t[i].inside;
            whole = whole && (!t[i].inside || (t[i].fx == 0.f && t[i].fy == 0.f));
        }
        float v[3][4];
        if (!any) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[0][i] = v[1][i] = v[2][i] = fill;
        } else if (whole) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float t00 = lut[s[t[i].o00 + c]];
                    v[c][i] = t[i].inside ? t00 : fill;
                }
        } else if (wide) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int at = min(t[i].o00, sample_bytes - 8), ab = min(t[i].o10, sample_bytes - 8);
                const unsigned long long wt = load_u64(s + at), wb = load_u64(s + ab);
                const unsigned w00 = (unsigned)(wt >> (8 * (t[i].o00 - at))), w01 = (unsigned)(wt >> (8 * (t[i].o01 - at)));
                const unsigned w10 = (unsigned)(wb >> (8 * (t[i].o10 - ab))), w11 = (unsigned)(wb >> (8 * (t[i].o11 - ab)));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float r = augment_blend(lut[(w00 >> (8 * c)) & 255u], lut[(w01 >> (8 * c)) & 255u], lut[(w10 >> (8 * c)) & 255u],
                                                  lut[(w11 >> (8 * c)) & 255u], t[i].fx, t[i].fy);
                    v[c][i] = t[i].inside ? r : fill;
                }
            }
        } else {  // a source of one or two pixels
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float r = augment_blend(lut[s[t[i].o00 + c]], lut[s[t[i].o01 + c]], lut[s[t[i].o10 + c]], lut[s[t[i].o11 + c]],
                                                  t[i].fx, t[i].fy);
                    v[c][i] = t[i].inside ? r : fill;
                }
        }
        if (kPhoto) {
            const bool clamp = norm.clamp != 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v0 = v[0][i], v1 = v[1][i], v2 = v[2][i];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float r = photo_channel(pp[3 * c], pp[3 * c + 1], pp[3 * c + 2], pp[9 + c], v0, v1, v2, clamp, norm.s[c], norm.t[c]);
                    v[c][i] = box[i] ? pp[16 + c] : (t[i].inside ? r : fill);
                }
            }
        }
        float* o = d + (size_t)y * W + x;
        if (kQuad) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *(float4*)(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c * plane + i] = v[c][i];
                }
        }
    }
}

// One half-size level of samples [first, first + count) of a dataset from the level before it: bytes in, bytes out, integers only.
//     y0 = 2y, y1 = min(2y + 1, Hp - 1), x0 = 2x, x1 = min(2x + 1, Wp - 1)
//     v  = (p[y0][x0] + p[y0][x1] + p[y1][x0] + p[y1][x1] + 2) >> 2
// A thread owns one output pixel (three channels) and strides over the pixels of a sample (blockIdx.x) and over the samples
// (blockIdx.y), so `count` is not limited by a grid dimension.  Offsets inside one sample fit an int (8192 * 8192 * 3); the sample bases
// are formed in 64 bits first.
__global__ __launch_bounds__(kBlock) void dataset_halve_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                   long long first, long long count, int Hp, int Wp, int H, int W) {
    const int pixels = H * W;
    const size_t src_bytes = (size_t)Hp * Wp * 3, dst_bytes = (size_t)pixels * 3;
    for (long long n = blockIdx.y; n < count; n += gridDim.y) {
        const unsigned char* s = src + (size_t)(first + n) * src_bytes;
        unsigned char* d = dst + (size_t)(first + n) * dst_bytes;
        for (int p = blockIdx.x * kBlock + threadIdx.x; p < pixels; p += gridDim.x * kBlock) {
            const int y = p / W, x = p - y * W;
            const int y0 = 2 * y, y1 = min(2 * y + 1, Hp - 1), x0 = 2 * x, x1 = min(2 * x + 1, Wp - 1);
            const int o00 = (y0 * Wp + x0) * 3, o01 = (y0 * Wp + x1) * 3, o10 = (y1 * Wp + x0) * 3, o11 = (y1 * Wp + x1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned v = (unsigned)s[o00 + c] + s[o01 + c] + s[o10 + c] + s[o11 + c] + 2u;
                d[3 * p + c] = (unsigned char)(v >> 2);
            }
        }
    }
}

bool dims_ok(int Hs, int Ws, int H, int W) { return Hs > 0 && Ws > 0 && H > 0 && W > 0 && Hs <= kMaxDim && Ws <= kMaxDim && H <= kMaxDim && W <= kMaxDim; }

// 2 x 3 affine maps in double, a[r][0] * x + a[r][1] * y + a[r][2]; compose(a, t) = a after t
struct Affine {
    double v[2][3];
};
Affine compose(const Affine& a, const Affine& t) {
    Affine r;
    for (int i = 0; i < 2; ++i) {
        r.v[i][0] = a.v[i][0] * t.v[0][0] + a.v[i][1] * t.v[1][0];
        r.v[i][1] = a.v[i][0] * t.v[0][1] + a.v[i][1] * t.v[1][1];
        r.v[i][2] = a.v[i][0] * t.v[0][2] + a.v[i][1] * t.v[1][2] + a.v[i][2];
    }
    return r;
}

// every instantiation there is, by what the job carries; .quad: W % 4 == 0 and dst 16-byte aligned.  (The order of the rows is the order of
// the eight kernels in the code object, which follows their first mention: reordering them reorders the object.)
using AugmentKernel = void (*)(const unsigned char*, const float*, const float*, float*, int, int, int, int, int, float, const float*, PhotoNorm,
                               ResidentArgs);
enum { kRowPhoto, kRowPlain, kRowLevels, kRowResident };
const struct {
    const char* name;
    AugmentKernel quad, px;
} kAugmentKernels[4] = {
    {"augment_u8_photo", augment_u8_kernel<true, true>, augment_u8_kernel<false, true>},
    {"augment_u8", augment_u8_kernel<true, false>, augment_u8_kernel<false, false>},
    {"augment_u8_resident_levels", augment_u8_kernel<true, true, true, true>, augment_u8_kernel<false, true, true, true>},
    {"augment_u8_resident", augment_u8_kernel<true, true, true>, augment_u8_kernel<false, true, true>},
};

// 3 x 4 affine colour maps in double, v[r][0..2] * rgb + v[r][3]; compose(l, a) = l after a
struct Colour {
    double v[3][4];
};
Colour compose(const Colour& l, const Colour& a) {
    Colour r;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r.v[i][j] = l.v[i][0] * a.v[0][j] + l.v[i][1] * a.v[1][j] + l.v[i][2] * a.v[2][j];
        r.v[i][3] = l.v[i][0] * a.v[0][3] + l.v[i][1] * a.v[1][3] + l.v[i][2] * a.v[2][3] + l.v[i][3];
    }
    return r;
}

}  // namespace

namespace cnn_amd {
// lut[v] = v * 1.f / 255 (data_format.cpp:19-21, the reference's own expression, evaluated on the host): one device copy per device,
// made at first use and kept for the life of the process
int device_lut(const float** out) {
    static std::mutex mu;
    static float* cached[64] = {nullptr};
    int dev = 0;
    CNN_HIP_CHECK(hipGetDevice(&dev));
    CNN_REQUIRE(dev >= 0 && dev < 64, "cnn_augment_u8: device index %d", dev);
    std::lock_guard<std::mutex> lk(mu);
    if (!cached[dev]) {
        float table[256];
        for (int v = 0; v < 256; ++v) table[v] = (unsigned char)v * 1.f / 255;
        float* p = nullptr;
        CNN_HIP_CHECK(hipMalloc((void**)&p, sizeof(table)));
        if (hipError_t e = hipMemcpy(p, table, sizeof(table), hipMemcpyHostToDevice)) {
            (void)hipFree(p);
            return fail(CNN_AMD_E_HIP + (int)e, "cnn_augment_u8: table upload failed: %s", hipGetErrorString(e));
        }
        cached[dev] = p;
    }
    *out = cached[dev];
    return CNN_AMD_OK;
}

// one launch per batch.  The stager (staging.hip) has checked a resident job's indices on the host.
int augment_u8_run(const char* who, const AugmentJob& j, hipStream_t s) {
    const ResidentArgs& r = j.res;
    const bool resident = r.indices != nullptr, levels = r.levels != nullptr;
    CNN_REQUIRE(j.src && j.mats && j.dst && (!resident || (r.labels && r.labels_out && j.photo)) && (!levels || (resident && r.table)),
                "%s: null pointer", who);
    CNN_REQUIRE(j.B > 0 && j.B <= kMaxDim && dims_ok(j.Hs, j.Ws, j.H, j.W), "%s: B=%d source %dx%d output %dx%d (each 1..%d)", who, j.B, j.Hs, j.Ws,
                j.H, j.W, kMaxDim);
    CNN_REQUIRE(!resident || (r.N > 0 && r.N <= 2147483647LL), "%s: N=%lld (1..2^31-1)", who, r.N);
    CNN_REQUIRE(!levels || (r.L > 1 && r.L <= kMaxLevels), "%s: levels=%d (2..%d)", who, r.L, kMaxLevels);
    CNN_REQUIRE(std::isfinite(j.fill), "%s: fill is not finite", who);
    const float* lut = nullptr;
    if (int rc = device_lut(&lut)) return rc;
    const int W4 = (j.W + 3) / 4;
    const int quads = j.H * W4;
    const int need = (quads + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(need < 4096 ? need : 4096), (unsigned)j.B);
    const bool quad = j.W % 4 == 0 && aligned16(j.dst);
    const auto& k = kAugmentKernels[levels ? kRowLevels : resident ? kRowResident : j.photo ? kRowPhoto : kRowPlain];
    char lv[16] = "";  // (the tag is only formatted while the kernel timer is on)
    if (levels && ktimer_active()) snprintf(lv, sizeof(lv), " L=%d", r.L);
    CNN_KLAUNCH(s, k.name, ((quad ? k.quad : k.px)<<<grid, kBlock, 0, s>>>(j.src, j.mats, lut, j.dst, j.Hs, j.Ws, j.H, j.W, W4, j.fill, j.photo, j.norm, r)),
                "B=%d src=%dx%d%s out=%dx%d %s", j.B, j.Hs, j.Ws, lv, j.H, j.W, quad ? "quad" : "px");
    return CNN_AMD_OK;
}

int dataset_halve_u8(const unsigned char* src, unsigned char* dst, long long first, long long count, int Hp, int Wp, hipStream_t stream) {
    CNN_REQUIRE(src && dst, "dataset_halve_u8: null pointer");
    CNN_REQUIRE(first >= 0 && count > 0 && Hp > 0 && Wp > 0 && Hp <= kMaxDim && Wp <= kMaxDim && (Hp > 1 || Wp > 1),
                "dataset_halve_u8: samples [%lld, +%lld) of %dx%d", first, count, Hp, Wp);
    const int H = (Hp + 1) / 2, W = (Wp + 1) / 2;
    const int need = (H * W + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(need < 4096 ? need : 4096), (unsigned)(count < 4096 ? count : 4096));
    CNN_KLAUNCH(stream, "dataset_halve_u8", (dataset_halve_u8_kernel<<<grid, kBlock, 0, stream>>>(src, dst, first, count, Hp, Wp, H, W)),
                "n=%lld src=%dx%d out=%dx%d", count, Hp, Wp, H, W);
    return CNN_AMD_OK;
}
}  // namespace cnn_amd

extern "C" {

int cnn_augment_u8(const unsigned char* src, int B, int Hs, int Ws, const float* matrices_dev, float fill, float* dst, int H, int W, void* stream) {
    return augment_u8_run("cnn_augment_u8", AugmentJob{src, B, Hs, Ws, matrices_dev, fill, dst, H, W, nullptr, PhotoNorm(), ResidentArgs()}, as_stream(stream));
}

// Host only.  The ops transform a canvas that starts as the source, in order, the way ImageAugmentor::make_augment transforms its cv::Mat;
// what is kept is the map from the current canvas back to the source.  Composed in double, rounded to fp32 once.
int cnn_augment_matrix(const cnn_augment_op* ops, int n_ops, int Hs, int Ws, int H, int W, float m[6]) {
    CNN_REQUIRE(m != nullptr && n_ops >= 0 && (ops != nullptr || n_ops == 0), "cnn_augment_matrix: null pointer");
    CNN_REQUIRE(dims_ok(Hs, Ws, H, W), "cnn_augment_matrix: source %dx%d output %dx%d (each 1..%d)", Hs, Ws, H, W, kMaxDim);
    Affine a = {{{1, 0, 0}, {0, 1, 0}}};
    double cw = Ws, ch = Hs;
    for (int i = 0; i < n_ops; ++i) {
        const cnn_augment_op& op = ops[i];
        Affine t = {{{1, 0, 0}, {0, 1, 0}}};
        switch (op.kind) {
        case CNN_AUG_HFLIP:
            t.v[0][0] = -1; t.v[0][2] = cw - 1;
            break;
        case CNN_AUG_VFLIP:
            t.v[1][1] = -1; t.v[1][2] = ch - 1;
            break;
        case CNN_AUG_CROP: {
            const double x0 = op.a, y0 = op.b, w = op.c, h = op.d;
            CNN_REQUIRE(std::isfinite(x0) && std::isfinite(y0) && std::isfinite(w) && std::isfinite(h), "cnn_augment_matrix: op %d: crop box is not finite", i);
            CNN_REQUIRE(x0 >= 0 && y0 >= 0 && w > 0 && h > 0 && x0 + w <= cw && y0 + h <= ch,
                        "cnn_augment_matrix: op %d: crop box x0=%g y0=%g w=%g h=%g outside the %gx%g canvas", i, x0, y0, w, h, ch, cw);
            t.v[0][2] = x0; t.v[1][2] = y0;
            cw = w; ch = h;
            break;
        }
        case CNN_AUG_ROTATE: {
            const double deg = op.a;
            CNN_REQUIRE(std::isfinite(deg), "cnn_augment_matrix: op %d: angle is not finite", i);
            double c, s;
            if (std::fmod(deg, 90.0) == 0.0) {  // quarter turns map integers to integers: sine and cosine from a table
                static const double kCos[4] = {1, 0, -1, 0}, kSin[4] = {0, 1, 0, -1};
                const int k = (int)std::fmod(std::fmod(deg / 90.0, 4.0) + 4.0, 4.0);
                c = kCos[k]; s = kSin[k];
            } else {
                const double rad = deg * 3.14159265358979323846 / 180.0;
                c = std::cos(rad); s = std::sin(rad);
            }
            // positive = counter-clockwise on the screen (cv::getRotationMatrix2D); this is the inverse map warpAffine applies
            const double cx = (cw - 1) / 2, cy = (ch - 1) / 2;
            t.v[0][0] = c; t.v[0][1] = -s; t.v[0][2] = cx - (c * cx - s * cy);
            t.v[1][0] = s; t.v[1][1] = c;  t.v[1][2] = cy - (s * cx + c * cy);
            break;
        }
        default:
            return fail(CNN_AMD_E_BADARG, "cnn_augment_matrix: op %d: unknown kind %d", i, op.kind);
        }
        a = compose(a, t);
    }
    // the resize of the canvas to W x H, half-pixel centres: sx = (x + 0.5) * cw / W - 0.5
    const double kx = cw / W, ky = ch / H;
    const Affine r = {{{kx, 0, 0.5 * kx - 0.5}, {0, ky, 0.5 * ky - 0.5}}};
    a = compose(a, r);
    for (int i = 0; i < 6; ++i) {
        m[i] = (float)(a.v[i / 3][i % 3] + 0.0);  // (+ 0.0: a product such as 0 * -1 leaves -0)
        CNN_REQUIRE(std::isfinite(m[i]), "cnn_augment_matrix: the composed map is not finite");
    }
    return CNN_AMD_OK;
}

// Host only.  How many levels a chain of half-size images has until both dimensions are 1; 0 (and a message) for sizes outside 1..8192.
int cnn_dataset_max_levels(int Hs, int Ws) {
    if (!(Hs > 0 && Ws > 0 && Hs <= kMaxDim && Ws <= kMaxDim)) {
        (void)fail(CNN_AMD_E_BADARG, "cnn_dataset_max_levels: %dx%d (each 1..%d)", Hs, Ws, kMaxDim);
        return 0;
    }
    int n = 1;
    for (int h = Hs, w = Ws; h > 1 || w > 1; h = (h + 1) / 2, w = (w + 1) / 2) ++n;
    return n;
}

// Host only.  The level a sample gathers from and its map on that level (include/cnn_amd.h has the rule; tests/mip_ref.py restates it).
// All in double; every product, sum and quotient rounded separately; the two offsets rounded to fp32 once.
int cnn_augment_level(const float m[6], int levels, int* level, float m_level[6]) {
#pragma clang fp contract(off)
    CNN_REQUIRE(m != nullptr && level != nullptr && m_level != nullptr, "cnn_augment_level: null pointer");
    CNN_REQUIRE(levels >= 1 && levels <= kMaxLevels, "cnn_augment_level: levels=%d (1..%d)", levels, kMaxLevels);
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const double rx = std::sqrt(m0 * m0 + m3 * m3), ry = std::sqrt(m1 * m1 + m4 * m4);
    const double r = rx > ry ? rx : ry;  // source pixels per output pixel
    int l = 0;
    if (std::isfinite(rx) && std::isfinite(ry))
        while (l + 1 < levels && r >= (double)(1 << (l + 1))) ++l;
    *level = l;
    if (l == 0) {
        memmove(m_level, m, 6 * sizeof(float));  // bit for bit
        return CNN_AMD_OK;
    }
    const double k = (double)(1 << l);
    m_level[0] = (float)(m0 / k);
    m_level[1] = (float)(m1 / k);
    m_level[2] = (float)((m2 + 0.5) / k - 0.5);
    m_level[3] = (float)(m3 / k);
    m_level[4] = (float)(m4 / k);
    m_level[5] = (float)((m5 + 0.5) / k - 0.5);
    return CNN_AMD_OK;
}

// Host only.  Each op is an affine map of the colour vector; they apply in order (op 0 first), with no clamp between them.  Composed in
// double, rounded to fp32 once: out[0..8] = A row-major, out[9..11] = o (the first twelve floats of a sample's photo block).
int cnn_colour_matrix(const cnn_colour_op* ops, int n_ops, float out[12]) {
    CNN_REQUIRE(out != nullptr && n_ops >= 0 && (ops != nullptr || n_ops == 0), "cnn_colour_matrix: null pointer");
    static const double kGray[3] = {0.299, 0.587, 0.114};
    // RGB -> YIQ; the rows of I and Q sum to zero, so the grey axis is the Y axis
    static const double kYiq[3][3] = {{0.299, 0.587, 0.114}, {0.5959, -0.2746, -0.3213}, {0.2115, -0.5227, 0.3112}};
    Colour a = {{{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}}};
    for (int i = 0; i < n_ops; ++i) {
        const cnn_colour_op& op = ops[i];
        const double f = op.a;
        Colour l = {{{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}}};
        CNN_REQUIRE(op.kind >= CNN_COL_BRIGHTNESS && op.kind <= CNN_COL_HUE, "cnn_colour_matrix: op %d: unknown kind %d", i, op.kind);
        CNN_REQUIRE(std::isfinite(f), "cnn_colour_matrix: op %d: argument is not finite", i);
        switch (op.kind) {
        case CNN_COL_BRIGHTNESS:
            for (int r = 0; r < 3; ++r) l.v[r][r] = f;
            break;
        case CNN_COL_CONTRAST: {
            const double pivot = op.b;
            CNN_REQUIRE(std::isfinite(pivot), "cnn_colour_matrix: op %d: pivot is not finite", i);
            for (int r = 0; r < 3; ++r) {
                l.v[r][r] = f;
                l.v[r][3] = (1 - f) * pivot;
            }
            break;
        }
        case CNN_COL_SATURATION:
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) l.v[r][c] = (r == c ? f : 0.0) + (1 - f) * kGray[c];
            break;
        default: {  // CNN_COL_HUE: I' = c*I - s*Q, Q' = s*I + c*Q, Y kept.  L = I + (c - 1) * P + s * K: the identity exactly at c = 1, s = 0
            double c, s;
            if (std::fmod(f, 90.0) == 0.0) {  // quarter turns: sine and cosine from a table (360 degrees is 0 degrees exactly)
                static const double kCos[4] = {1, 0, -1, 0}, kSin[4] = {0, 1, 0, -1};
                const int k = (int)std::fmod(std::fmod(f / 90.0, 4.0) + 4.0, 4.0);
                c = kCos[k]; s = kSin[k];
            } else {
                const double rad = f * 3.14159265358979323846 / 180.0;
                c = std::cos(rad); s = std::sin(rad);
            }
            const double (&t)[3][3] = kYiq;
            const double det = t[0][0] * (t[1][1] * t[2][2] - t[1][2] * t[2][1]) - t[0][1] * (t[1][0] * t[2][2] - t[1][2] * t[2][0]) +
                               t[0][2] * (t[1][0] * t[2][1] - t[1][1] * t[2][0]);
            double inv[3][3];  // YIQ -> RGB: the inverse of the table, not the rounded textbook constants
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) {
                    const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, q1 = (q + 1) % 3, q2 = (q + 2) % 3;
                    inv[r][q] = (t[q1][r1] * t[q2][r2] - t[q1][r2] * t[q2][r1]) / det;
                }
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) {
                    const double p = inv[r][1] * t[1][q] + inv[r][2] * t[2][q];   // the projection on the chroma plane
                    const double k = inv[r][2] * t[1][q] - inv[r][1] * t[2][q];   // a quarter turn in it
                    l.v[r][q] = (r == q ? 1.0 : 0.0) + ((c - 1) * p + s * k);
                }
            break;
        }
        }
        a = compose(l, a);
    }
    for (int i = 0; i < 12; ++i) {
        out[i] = (float)((i < 9 ? a.v[i / 3][i % 3] : a.v[i - 9][3]) + 0.0);  // (+ 0.0: a product such as 0 * -1 leaves -0)
        CNN_REQUIRE(std::isfinite(out[i]), "cnn_colour_matrix: the composed map is not finite");
    }
    return CNN_AMD_OK;
}

}  // extern "C"
