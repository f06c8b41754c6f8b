// layerwise.hip -- layer-wise adaptive optimizers on the flat arena: the deterministic segmented norm (cnn_segment_norms), LAMB
// (cnn_lamb_update) and LARS (cnn_lars_update).  include/cnn_amd.h has the formulas, common.h the one-element functions.
//
// Every streaming kernel here has ONE shape (walk_chunk): workgroup b owns the chunk [b * kChunk, (b + 1) * kChunk) of the flat range,
// kChunk = 1024 = one float4 per lane.  It issues its float4 loads first, then finds the segment of its first element by a binary
// search in the device table (wave-uniform: scalar loads, under the vector loads in flight), and then
//   * the chunk lies inside ONE segment (nearly all of them: segments are layers' tensors): the lanes work on the float4 they hold;
//     a norm's partial is the lane's four squares, the wave's shuffle tree, the four waves in order -> the slot of (segment, chunk);
//   * otherwise (a segment boundary inside the chunk, or the last, shorter chunk): the waves take the (segment, chunk) overlaps in
//     turn, each overlap lane-strided by one wave, scalar loads -> the same slot.
// Per-segment flags and ratios are wave-uniform in both forms: no element ever looks its segment up.  The slots of a segment are
// consecutive (slot_base[s] + chunk - first chunk of s); seg_finish adds them in ascending order, one wave per segment.  The element
// -> lane assignment is the same with float4 and with scalar loads (unaligned pointers), so the sums do not depend on alignment.
#include <cmath>
#include <cstdint>
#include <vector>

#include "common.h"

using namespace cnn_amd;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kChunk = CNN_SEG_CHUNK;
static_assert(kChunk == 4 * kBlock, "one float4 per lane");

struct SegTable {
    const uint32_t* bounds;     // nseg + 1
    const uint32_t* flags;      // nseg
    const uint32_t* slot_base;  // nseg + 1: first partial slot of every segment, the last value is the number of slots
    uint32_t nseg, n;
};

// the segment that holds element idx (< n): the first s with bounds[s + 1] > idx
__device__ __forceinline__ uint32_t seg_of(const SegTable& t, uint32_t idx) {
    uint32_t lo = 0, hi = t.nseg - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t.bounds[mid + 1] > idx) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_down(x, off, kWave);
    return x;  // (valid in lane 0)
}

// both sums of the workgroup, the waves added in order (valid in thread 0)
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
        lds[2 * wave] = a;
        lds[2 * wave + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = lds[0];
        b = lds[1];
        for (int w = 1; w < kWaves; ++w) {
            a += lds[2 * w];
            b += lds[2 * w + 1];
        }
    }
}

template <bool kVec>
__device__ __forceinline__ float4 load4(const float* p, uint32_t e) {
    if (kVec) return *(const float4*)(p + e);
    return float4{p[e], p[e + 1], p[e + 2], p[e + 3]};
}
template <bool kVec>
__device__ __forceinline__ void store4(float* p, uint32_t e, const float4& q) {
    if (kVec) {
        *(float4*)(p + e) = q;
    } else {
        p[e] = q.x; p[e + 1] = q.y; p[e + 2] = q.z; p[e + 3] = q.w;
    }
}
__device__ __forceinline__ void add_sq(double& acc, float x) {
    const double d = (double)x;
    acc += d * d;  // (the product of two fp32 values is exact in fp64)
}

// Op: Regs; load<kVec>(Regs&, e) the four elements from e; begin(s) this segment's uniform values; run4(Regs&, a, b) the work on
// them, squares added to a / b in element order; store<kVec>(Regs&, e); one(i, a, b) the same for one element; put(slot, a, b)
// (kSums only).
template <bool kVec, class Op>
__device__ __forceinline__ void walk_chunk(const SegTable& t, Op& op, double* lds) {
    const uint32_t c0 = blockIdx.x * kChunk;  // (< n <= 2^32 - 257: the grid is ceil(n / kChunk))
    const bool full = t.n - c0 >= kChunk;
    const uint32_t c1 = full ? c0 + kChunk : t.n;
    const uint32_t e = c0 + 4 * threadIdx.x;
    typename Op::Regs r;
    if (full) op.template load<kVec>(r, e);
    const uint32_t s0 = seg_of(t, c0);
    if (full && t.bounds[s0 + 1] >= c1) {
        op.begin(s0);
        double a = 0.0, b = 0.0;
        op.run4(r, a, b);
        op.template store<kVec>(r, e);
        if (Op::kSums) {
            block_sum2(a, b, lds);
            if (threadIdx.x == 0) op.put(t.slot_base[s0] + (blockIdx.x - t.bounds[s0] / kChunk), a, b);
        }
        return;
    }
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    for (uint32_t s = s0 + wave; s < t.nseg; s += kWaves) {
        const uint32_t sb = t.bounds[s];
        if (sb >= c1) break;
        const uint32_t se = t.bounds[s + 1];
        const uint32_t lo = sb > c0 ? sb : c0, hi = se < c1 ? se : c1;
        op.begin(s);
        double a = 0.0, b = 0.0;
        for (uint32_t i = lo + lane; i < hi; i += kWave) op.one(i, a, b);
        if (Op::kSums) {
            a = wave_sum(a);
            b = wave_sum(b);
            if (lane == 0) op.put(t.slot_base[s] + (blockIdx.x - sb / kChunk), a, b);
        }
    }
}

// ---- the norm of one array (cnn_segment_norms), of two arrays (cnn_lars_update: parameters and gradients) -------------------------
template <bool kTwo>
struct NormOp {
    static constexpr bool kSums = true;
    const float* x;
    const float* y;
    double* pa;
    double* pb;
    struct Regs { float4 x, y; };
    template <bool kVec>
    __device__ __forceinline__ void load(Regs& r, uint32_t e) const {
        r.x = load4<kVec>(x, e);
        if (kTwo) r.y = load4<kVec>(y, e);
    }
    __device__ __forceinline__ void begin(uint32_t) {}
    __device__ __forceinline__ void run4(Regs& r, double& a, double& b) const {
        add_sq(a, r.x.x); add_sq(a, r.x.y); add_sq(a, r.x.z); add_sq(a, r.x.w);
        if (kTwo) { add_sq(b, r.y.x); add_sq(b, r.y.y); add_sq(b, r.y.z); add_sq(b, r.y.w); }
    }
    template <bool kVec>
    __device__ __forceinline__ void store(Regs&, uint32_t) const {}
    __device__ __forceinline__ void one(uint32_t i, double& a, double& b) const {
        add_sq(a, x[i]);
        if (kTwo) add_sq(b, y[i]);
    }
    __device__ __forceinline__ void put(uint32_t slot, double a, double b) const {
        pa[slot] = a;
        if (kTwo) pb[slot] = b;
    }
};

// ---- LAMB, first pass: moments, r -> update, partial sums of |p|^2 and |r|^2 ------------------------------------------------------
struct LambMomentsOp {
    static constexpr bool kSums = true;
    const float* p;
    const float* g;
    float* m;
    float* v;
    float* upd;
    double* pa;
    double* pb;
    const uint32_t* flags;
    LambScalars s;
    bool decay;
    struct Regs { float4 p, g, m, v; };
    template <bool kVec>
    __device__ __forceinline__ void load(Regs& r, uint32_t e) const {
        r.p = load4<kVec>(p, e);
        r.g = load4<kVec>(g, e);
        r.m = load4<kVec>(m, e);
        r.v = load4<kVec>(v, e);
    }
    __device__ __forceinline__ void begin(uint32_t seg) { decay = (flags[seg] & CNN_SEG_DECAY) != 0 && s.wd != 0.f; }
    __device__ __forceinline__ void run4(Regs& r, double& a, double& b) const {
        add_sq(a, r.p.x); add_sq(a, r.p.y); add_sq(a, r.p.z); add_sq(a, r.p.w);
        r.g.x = lamb_moments_one(r.p.x, r.g.x, r.m.x, r.v.x, s, decay);  // (g now holds r)
        r.g.y = lamb_moments_one(r.p.y, r.g.y, r.m.y, r.v.y, s, decay);
        r.g.z = lamb_moments_one(r.p.z, r.g.z, r.m.z, r.v.z, s, decay);
        r.g.w = lamb_moments_one(r.p.w, r.g.w, r.m.w, r.v.w, s, decay);
        add_sq(b, r.g.x); add_sq(b, r.g.y); add_sq(b, r.g.z); add_sq(b, r.g.w);
    }
    template <bool kVec>
    __device__ __forceinline__ void store(Regs& r, uint32_t e) const {
        store4<kVec>(m, e, r.m);
        store4<kVec>(v, e, r.v);
        store4<kVec>(upd, e, r.g);
    }
    __device__ __forceinline__ void one(uint32_t i, double& a, double& b) const {
        const float pi = p[i];
        float mi = m[i], vi = v[i];
        const float ri = lamb_moments_one(pi, g[i], mi, vi, s, decay);
        m[i] = mi;
        v[i] = vi;
        upd[i] = ri;
        add_sq(a, pi);
        add_sq(b, ri);
    }
    __device__ __forceinline__ void put(uint32_t slot, double a, double b) const {
        pa[slot] = a;
        pb[slot] = b;
    }
};

// ---- LAMB, second pass: p -= lr * (ratio[s] * r) ----------------------------------------------------------------------------------
struct LambApplyOp {
    static constexpr bool kSums = false;
    float* p;
    const float* upd;
    float* keep;  // nullable
    const float* ratios;
    float lr, ratio;
    struct Regs { float4 p, r; };
    template <bool kVec>
    __device__ __forceinline__ void load(Regs& r, uint32_t e) const {
        r.p = load4<kVec>(p, e);
        r.r = load4<kVec>(upd, e);
    }
    __device__ __forceinline__ void begin(uint32_t seg) { ratio = ratios[seg]; }
    __device__ __forceinline__ void run4(Regs& r, double&, double&) const {
        r.r.x = lamb_apply_one(r.p.x, r.r.x, ratio, lr);  // (r now holds p')
        r.r.y = lamb_apply_one(r.p.y, r.r.y, ratio, lr);
        r.r.z = lamb_apply_one(r.p.z, r.r.z, ratio, lr);
        r.r.w = lamb_apply_one(r.p.w, r.r.w, ratio, lr);
    }
    template <bool kVec>
    __device__ __forceinline__ void store(Regs& r, uint32_t e) const {
        if (keep) store4<kVec>(keep, e, r.p);
        store4<kVec>(p, e, r.r);
    }
    __device__ __forceinline__ void one(uint32_t i, double&, double&) const {
        const float pi = p[i];
        if (keep) keep[i] = pi;
        p[i] = lamb_apply_one(pi, upd[i], ratio, lr);
    }
    __device__ __forceinline__ void put(uint32_t, double, double) const {}
};

// ---- LARS, the step: sgdm_vec's streams with the segment's ratio -------------------------------------------------------------------
struct LarsArgs {
    float lr, momentum, wd, scale;
    bool scaled, nesterov;
};
template <bool kMomentum>
struct LarsApplyOp {
    static constexpr bool kSums = false;
    float* p;
    const float* g;
    float* v;
    float* keep;  // nullable
    const float* ratios;
    const uint32_t* flags;
    LarsArgs a;
    float ratio;
    bool decay;
    struct Regs { float4 p, g, v; };
    template <bool kVec>
    __device__ __forceinline__ void load(Regs& r, uint32_t e) const {
        r.p = load4<kVec>(p, e);
        r.g = load4<kVec>(g, e);
        if (kMomentum) r.v = load4<kVec>(v, e);
        else r.v = float4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void begin(uint32_t seg) {
        ratio = ratios[seg];
        decay = (flags[seg] & CNN_SEG_DECAY) != 0 && a.wd != 0.f;
    }
    __device__ __forceinline__ void run4(Regs& r, double&, double&) const {
        r.g.x = lars_one<kMomentum>(r.p.x, r.g.x, r.v.x, ratio, a.lr, a.momentum, a.wd, a.scale, a.scaled, decay, a.nesterov);  // (g now holds p')
        r.g.y = lars_one<kMomentum>(r.p.y, r.g.y, r.v.y, ratio, a.lr, a.momentum, a.wd, a.scale, a.scaled, decay, a.nesterov);
        r.g.z = lars_one<kMomentum>(r.p.z, r.g.z, r.v.z, ratio, a.lr, a.momentum, a.wd, a.scale, a.scaled, decay, a.nesterov);
        r.g.w = lars_one<kMomentum>(r.p.w, r.g.w, r.v.w, ratio, a.lr, a.momentum, a.wd, a.scale, a.scaled, decay, a.nesterov);
    }
    template <bool kVec>
    __device__ __forceinline__ void store(Regs& r, uint32_t e) const {
        if (keep) store4<kVec>(keep, e, r.p);
        store4<kVec>(p, e, r.g);
        if (kMomentum) store4<kVec>(v, e, r.v);
    }
    __device__ __forceinline__ void one(uint32_t i, double&, double&) const {
        const float pi = p[i];
        float vel = kMomentum ? v[i] : 0.f;
        if (keep) keep[i] = pi;
        p[i] = lars_one<kMomentum>(pi, g[i], vel, ratio, a.lr, a.momentum, a.wd, a.scale, a.scaled, decay, a.nesterov);
        if (kMomentum) v[i] = vel;
    }
    __device__ __forceinline__ void put(uint32_t, double, double) const {}
};

template <bool kVec, class Op>
__global__ __launch_bounds__(kBlock) void seg_walk(const SegTable t, Op op) {
    __shared__ double lds[2 * kWaves];
    walk_chunk<kVec>(t, op, lds);
}

// ---- the finish: one wave per segment adds the segment's slots (each lane its strided share in ascending order, then the tree) -----
enum FinishMode { kFinishNorms = 0, kFinishLamb = 1, kFinishLars = 2 };
struct FinishArgs {
    float* out;  // kFinishNorms: norms[nseg]; otherwise stats[3 * nseg]
    float wd, trust, eps, scale;
    bool scaled;
};
template <int kMode>
__device__ __forceinline__ void finish_segment(const SegTable& t, const FinishArgs& f, uint32_t s, double a, double b) {
#pragma clang fp contract(off)
    const float w = (float)sqrt(a);
    if (kMode == kFinishNorms) {
        f.out[s] = w;
        return;
    }
    const float un = (float)sqrt(b);
    const uint32_t fl = t.flags[s];
    const bool adapt = (fl & CNN_SEG_ADAPT) != 0;
    float u = un, ratio = 1.f;
    if (kMode == kFinishLamb) {
        if (adapt && w > 0.f && u > 0.f) ratio = w / u;
    } else {
        u = f.scaled ? un * f.scale : un;
        const float wds = (fl & CNN_SEG_DECAY) ? f.wd : 0.f;
        if (adapt && w > 0.f && u > 0.f) {
            const float num = f.trust * w;
            const float ww = wds * w;
            const float s1 = u + ww;
            const float den = s1 + f.eps;
            ratio = num / den;
        }
    }
    f.out[s] = w;
    f.out[t.nseg + s] = u;
    f.out[2 * (size_t)t.nseg + s] = ratio;
}

template <int kMode>
__global__ __launch_bounds__(kBlock) void seg_finish(const SegTable t, const double* __restrict__ pa, const double* __restrict__ pb,
                                                     const FinishArgs f) {
    const uint32_t s = blockIdx.x * kWaves + threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (s >= t.nseg) return;  // (no barrier below)
    const uint32_t base = t.slot_base[s], cnt = t.slot_base[s + 1] - base;
    double a = 0.0, b = 0.0;
    for (uint32_t i = lane; i < cnt; i += kWave) {
        a += pa[base + i];
        if (kMode != kFinishNorms) b += pb[base + i];
    }
    a = wave_sum(a);
    if (kMode != kFinishNorms) b = wave_sum(b);
    if (lane != 0) return;
    finish_segment<kMode>(t, f, s, a, b);
}

// ---- the handle -------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kMagic = 0x434e4e4c41594552ull;  // "CNNLAYER"
struct Layerwise {
    uint64_t magic;
    SegTable t;
    uint32_t* table_dev;  // bounds, flags, slot_base in one allocation
    double* partial;      // 2 * n_slots
    float* stats;         // 3 * nseg
    uint32_t n_slots, n_chunks;
};

inline Layerwise* as_handle(void* h) {
    Layerwise* lw = (Layerwise*)h;
    return (lw != nullptr && lw->magic == kMagic) ? lw : nullptr;
}

template <class Op>
int launch_walk(const Layerwise* lw, const Op& op, bool vec, const char* name, hipStream_t s) {
    if (vec) {
        CNN_KLAUNCH(s, name, (seg_walk<true, Op><<<lw->n_chunks, kBlock, 0, s>>>(lw->t, op)), "n=%u segments=%u", lw->t.n, lw->t.nseg);
    } else {
        CNN_KLAUNCH(s, name, (seg_walk<false, Op><<<lw->n_chunks, kBlock, 0, s>>>(lw->t, op)), "scalar n=%u segments=%u", lw->t.n, lw->t.nseg);
    }
    return CNN_AMD_OK;
}

template <int kMode>
int launch_finish(const Layerwise* lw, const FinishArgs& f, hipStream_t s) {
    const unsigned grid = (lw->t.nseg + kWaves - 1) / kWaves;
    CNN_KLAUNCH(s, "seg_finish", (seg_finish<kMode><<<grid, kBlock, 0, s>>>(lw->t, lw->partial, lw->partial + lw->n_slots, f)), "segments=%u slots=%u",
                lw->t.nseg, lw->n_slots);
    return CNN_AMD_OK;
}

}  // namespace

extern "C" {

int cnn_layerwise_create(const uint32_t* seg_bounds, const uint32_t* seg_flags, size_t n_segments, void** handle) {
    CNN_REQUIRE(seg_bounds && seg_flags && handle, "cnn_layerwise_create: null pointer");
    *handle = nullptr;
    CNN_REQUIRE(n_segments >= 1 && n_segments <= (size_t)0xFFFFFFFFu - 4 * kWave, "cnn_layerwise_create: n_segments=%zu", n_segments);
    CNN_REQUIRE(seg_bounds[0] == 0, "cnn_layerwise_create: seg_bounds[0]=%u, the first segment starts at 0", seg_bounds[0]);
    for (size_t s = 0; s < n_segments; ++s) {
        CNN_REQUIRE(seg_bounds[s + 1] > seg_bounds[s], "cnn_layerwise_create: segment %zu = [%u, %u) is empty or unsorted", s, seg_bounds[s],
                    seg_bounds[s + 1]);
        CNN_REQUIRE((seg_flags[s] & ~(CNN_SEG_DECAY | CNN_SEG_ADAPT)) == 0, "cnn_layerwise_create: seg_flags[%zu]=%#x has unknown bits", s, seg_flags[s]);
    }
    const uint32_t n = seg_bounds[n_segments];
    CNN_REQUIRE(n <= 0xFFFFFFFFu - 4 * kWave, "cnn_layerwise_create: n=%u exceeds 2^32 - 257: step the arena in pieces", n);
    // bounds | flags | slot_base
    std::vector<uint32_t> table(3 * n_segments + 2);
    uint64_t slots = 0;
    for (size_t s = 0; s < n_segments; ++s) {
        table[s] = seg_bounds[s];
        table[n_segments + 1 + s] = seg_flags[s];
        table[2 * n_segments + 1 + s] = (uint32_t)slots;
        slots += (uint64_t)((seg_bounds[s + 1] - 1) / kChunk - seg_bounds[s] / kChunk + 1);
        CNN_REQUIRE(slots <= 0xFFFFFFFFull, "cnn_layerwise_create: %zu segments over n=%u need more than 2^32 partial sums", n_segments, n);
    }
    table[n_segments] = n;
    table[3 * n_segments + 1] = (uint32_t)slots;
    Layerwise* lw = new Layerwise();
    auto fail_free = [&](hipError_t e, const char* what) {
        if (lw->table_dev) (void)hipFree(lw->table_dev);
        if (lw->partial) (void)hipFree(lw->partial);
        if (lw->stats) (void)hipFree(lw->stats);
        delete lw;
        return fail(CNN_AMD_E_HIP + (int)e, "cnn_layerwise_create: %s failed: %s", what, hipGetErrorString(e));
    };
    hipError_t e = hipMalloc((void**)&lw->table_dev, sizeof(uint32_t) * table.size());
    if (e != hipSuccess) { lw->table_dev = nullptr; return fail_free(e, "hipMalloc(table)"); }
    e = hipMalloc((void**)&lw->partial, sizeof(double) * 2 * (size_t)slots);
    if (e != hipSuccess) { lw->partial = nullptr; return fail_free(e, "hipMalloc(partials)"); }
    e = hipMalloc((void**)&lw->stats, sizeof(float) * 3 * n_segments);
    if (e != hipSuccess) { lw->stats = nullptr; return fail_free(e, "hipMalloc(stats)"); }
    e = hipMemcpy(lw->table_dev, table.data(), sizeof(uint32_t) * table.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail_free(e, "hipMemcpy(table)");
    e = hipMemset(lw->stats, 0, sizeof(float) * 3 * n_segments);
    if (e != hipSuccess) return fail_free(e, "hipMemset(stats)");
    e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail_free(e, "hipDeviceSynchronize");
    lw->magic = kMagic;
    lw->t.bounds = lw->table_dev;
    lw->t.flags = lw->table_dev + n_segments + 1;
    lw->t.slot_base = lw->table_dev + 2 * n_segments + 1;
    lw->t.nseg = (uint32_t)n_segments;
    lw->t.n = n;
    lw->n_slots = (uint32_t)slots;
    lw->n_chunks = (n - 1) / kChunk + 1;
    *handle = lw;
    return CNN_AMD_OK;
}

int cnn_layerwise_destroy(void* handle) {
    Layerwise* lw = as_handle(handle);
    CNN_REQUIRE(lw != nullptr, "cnn_layerwise_destroy: not a handle of cnn_layerwise_create");
    lw->magic = 0;
    const hipError_t e1 = hipFree(lw->table_dev), e2 = hipFree(lw->partial), e3 = hipFree(lw->stats);
    delete lw;
    CNN_HIP_CHECK(e1);
    CNN_HIP_CHECK(e2);
    CNN_HIP_CHECK(e3);
    return CNN_AMD_OK;
}

int cnn_layerwise_stats(void* handle, float** stats_dev) {
    Layerwise* lw = as_handle(handle);
    CNN_REQUIRE(lw != nullptr && stats_dev != nullptr, "cnn_layerwise_stats: null pointer / not a handle of cnn_layerwise_create");
    *stats_dev = lw->stats;
    return CNN_AMD_OK;
}

int cnn_segment_norms(void* handle, const float* x, float* norms_dev, void* stream) {
    hipStream_t s = as_stream(stream);
    Layerwise* lw = as_handle(handle);
    CNN_REQUIRE(lw != nullptr, "cnn_segment_norms: not a handle of cnn_layerwise_create");
    CNN_REQUIRE(x && norms_dev, "cnn_segment_norms: null pointer");
    NormOp<false> op{x, nullptr, lw->partial, nullptr};
    if (int rc = launch_walk(lw, op, aligned16(x), "seg_norm_partial", s)) return rc;
    return launch_finish<kFinishNorms>(lw, FinishArgs{norms_dev, 0.f, 0.f, 0.f, 1.f, false}, s);
}

int cnn_lamb_update(void* handle, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* update, const cnn_lamb_options* opt,
                    float grad_scale, float* previous, void* stream) {
    hipStream_t s = as_stream(stream);
    Layerwise* lw = as_handle(handle);
    CNN_REQUIRE(lw != nullptr, "cnn_lamb_update: not a handle of cnn_layerwise_create");
    CNN_REQUIRE(params && grads && exp_avg && exp_avg_sq && update && opt, "cnn_lamb_update: null pointer");
    CNN_REQUIRE(opt->beta1 >= 0.f && opt->beta1 < 1.f && opt->beta2 >= 0.f && opt->beta2 < 1.f, "cnn_lamb_update: beta1=%g beta2=%g outside [0, 1)",
                (double)opt->beta1, (double)opt->beta2);
    CNN_REQUIRE(opt->eps > 0.f, "cnn_lamb_update: eps=%g must be positive", (double)opt->eps);
    CNN_REQUIRE(opt->weight_decay >= 0.f, "cnn_lamb_update: weight_decay=%g", (double)opt->weight_decay);
    CNN_REQUIRE(opt->step != 0, "cnn_lamb_update: step=0 (the number of this step, counted from 1)");
    LambScalars a;
    {
#pragma clang fp contract(off)
        a.beta1 = opt->beta1;
        a.beta2 = opt->beta2;
        a.omb1 = 1.f - opt->beta1;
        a.omb2 = 1.f - opt->beta2;
        a.eps = opt->eps;
        a.wd = opt->weight_decay;
        const double t = (double)opt->step;
        a.bc2s = (float)std::sqrt(1.0 - std::pow((double)opt->beta2, t));
        a.bc1 = (float)(1.0 - std::pow((double)opt->beta1, t));
        a.scale = grad_scale;
        a.scaled = grad_scale != 1.0f;
    }
    const bool vec1 = aligned16(params) && aligned16(grads) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(update);
    LambMomentsOp mo{params, grads, exp_avg, exp_avg_sq, update, lw->partial, lw->partial + lw->n_slots, lw->t.flags, a, false};
    if (int rc = launch_walk(lw, mo, vec1, "lamb_moments", s)) return rc;
    if (int rc = launch_finish<kFinishLamb>(lw, FinishArgs{lw->stats, 0.f, 0.f, 0.f, 1.f, false}, s)) return rc;
    const bool vec2 = aligned16(params) && aligned16(update) && (previous == nullptr || aligned16(previous));
    LambApplyOp ao{params, update, previous, lw->stats + 2 * (size_t)lw->t.nseg, opt->lr, 1.f};
    return launch_walk(lw, ao, vec2, "lamb_apply", s);
}

int cnn_lars_update(void* handle, float* params, const float* grads, float* velocity, const cnn_lars_options* opt, float grad_scale, float* previous,
                    void* stream) {
    hipStream_t s = as_stream(stream);
    Layerwise* lw = as_handle(handle);
    CNN_REQUIRE(lw != nullptr, "cnn_lars_update: not a handle of cnn_layerwise_create");
    CNN_REQUIRE(params && grads && opt, "cnn_lars_update: null pointer");
    CNN_REQUIRE(opt->momentum >= 0.f && opt->weight_decay >= 0.f, "cnn_lars_update: momentum=%g weight_decay=%g", (double)opt->momentum,
                (double)opt->weight_decay);
    CNN_REQUIRE(opt->trust_coefficient > 0.f, "cnn_lars_update: trust_coefficient=%g must be positive", (double)opt->trust_coefficient);
    CNN_REQUIRE(opt->eps > 0.f, "cnn_lars_update: eps=%g must be positive", (double)opt->eps);
    CNN_REQUIRE(velocity || opt->momentum == 0.f, "cnn_lars_update: null velocity with momentum=%g", (double)opt->momentum);
    const bool scaled = grad_scale != 1.0f, mom = opt->momentum != 0.f;
    NormOp<true> no{params, grads, lw->partial, lw->partial + lw->n_slots};
    if (int rc = launch_walk(lw, no, aligned16(params) && aligned16(grads), "lars_norms", s)) return rc;
    if (int rc = launch_finish<kFinishLars>(lw, FinishArgs{lw->stats, opt->weight_decay, opt->trust_coefficient, opt->eps, grad_scale, scaled}, s)) return rc;
    const LarsArgs a{opt->lr, opt->momentum, opt->weight_decay, grad_scale, scaled, opt->nesterov != 0};
    const bool vec = aligned16(params) && aligned16(grads) && (!mom || aligned16(velocity)) && (previous == nullptr || aligned16(previous));
    const float* ratios = lw->stats + 2 * (size_t)lw->t.nseg;
    if (mom) {
        LarsApplyOp<true> ao{params, grads, velocity, previous, ratios, lw->t.flags, a, 1.f, false};
        return launch_walk(lw, ao, vec, "lars_apply", s);
    }
    LarsApplyOp<false> ao{params, grads, velocity, previous, ratios, lw->t.flags, a, 1.f, false};
    return launch_walk(lw, ao, vec, "lars_apply", s);
}

}  // extern "C"
