// augment.hip -- geometric augmentation of uint8 image batches on the device (an addition: the reference's ImageAugmentor runs OpenCV on
// the host, pipeline.cpp:40-77): flip, crop, rotate and the resize to the network's size as ONE per-sample affine gather, fused with the
// bytes -> fp32 planar conversion the u8 stager does anyway (abi.hip, u8hwc_to_f32chw).  Decode stays on the host.
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
// quarter turns are bit-identical to the plain conversion of the permuted image.  There is no antialiasing: a large shrink ratio aliases.
#include <cmath>
#include <mutex>

#include "common.h"

using namespace cnn_amd;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 8192;  // fp32 holds every pixel index (and index + 0.5) below this exactly

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
template <bool kQuad>
__global__ __launch_bounds__(kBlock) void augment_u8_kernel(const unsigned char* __restrict__ src, const float* __restrict__ mats,
                                                            const float* __restrict__ lut_g, float* __restrict__ dst, int Hs, int Ws, int H,
                                                            int W, int W4, float fill) {
    __shared__ float lut[256];
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
    const size_t b = blockIdx.y;
    const float* m = mats + 6 * b;
    const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const unsigned char* s = src + b * 3 * ((size_t)Hs * Ws);
    const size_t plane = (size_t)H * W;
    float* d = dst + b * 3 * plane;
    const int quads = H * W4;
    const int sample_bytes = Hs * Ws * 3;
    const bool wide = sample_bytes >= 8;
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < quads; q += gridDim.x * kBlock) {
        const int y = q / W4, x = (q - y * W4) * 4;
        Taps t[4];
        bool any = false, whole = true;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            t[i] = augment_taps(m0, m1, m2, m3, m4, m5, x + i, y, Hs, Ws);
            t[i].inside = t[i].inside && (kQuad || x + i < W);
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

}  // namespace

extern "C" {

int cnn_augment_u8(const unsigned char* src, int B, int Hs, int Ws, const float* matrices_dev, float fill, float* dst, int H, int W, void* stream) {
    CNN_REQUIRE(src && matrices_dev && dst, "cnn_augment_u8: null pointer");
    CNN_REQUIRE(B > 0 && B <= kMaxDim && dims_ok(Hs, Ws, H, W), "cnn_augment_u8: B=%d source %dx%d output %dx%d (each 1..%d)", B, Hs, Ws, H, W, kMaxDim);
    CNN_REQUIRE(std::isfinite(fill), "cnn_augment_u8: fill is not finite");
    const float* lut = nullptr;
    if (int rc = device_lut(&lut)) return rc;
    hipStream_t s = as_stream(stream);
    const int W4 = (W + 3) / 4;
    const int quads = H * W4;
    const int need = (quads + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(need < 4096 ? need : 4096), (unsigned)B);
    if (W % 4 == 0 && aligned16(dst))
        CNN_KLAUNCH(s, "augment_u8", (augment_u8_kernel<true><<<grid, kBlock, 0, s>>>(src, matrices_dev, lut, dst, Hs, Ws, H, W, W4, fill)),
                    "B=%d src=%dx%d out=%dx%d quad", B, Hs, Ws, H, W);
    else
        CNN_KLAUNCH(s, "augment_u8", (augment_u8_kernel<false><<<grid, kBlock, 0, s>>>(src, matrices_dev, lut, dst, Hs, Ws, H, W, W4, fill)),
                    "B=%d src=%dx%d out=%dx%d px", B, Hs, Ws, H, W);
    return CNN_AMD_OK;
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

}  // extern "C"
