// elementwise.hip -- HBM-bound streaming kernels: ReLU fwd/bwd (relu.cpp:21-26,35-40), dropout, the SGD step (conv2d.cpp:205-217,
// linear.cpp:95-102), the optimizer steps, the clip, the gradient accumulation, the parameter average and the buffer exchange on the
// flat arena (additions), mixup / CutMix of a batch and the soft target rows (additions), and the softmax / cross-entropy and Grad-CAM glue (func.cpp:16-73, alexnet.cpp:107-140), which have shapes
// of their own.
//
// Every streaming kernel here has ONE shape (stream_walk) over the flat range [0, n):
//   * the float4 form (every pointer 16-byte aligned): workgroup 0 first takes the n % 4 trailing elements, one per lane, then every
//     lane grid-strides over the n / 4 float4 -- 16 B per lane and stream, consecutive lanes on consecutive float4;
//   * the scalar form (any alignment): a grid-stride loop over the elements from `begin`.
// A rule is an Op: the streams' pointers, the rule's scalars, and ONE member run<V>(i) that says what happens at index i of the
// streams taken as V = float (element i) or V = float4 (elements 4i .. 4i + 3): load the streams with at<V>, hand the values to the
// one-element arithmetic with each<V> / each_bit<V> (once, or on x, y, z, w in that order), store.  A rule's kernels are two named
// one-line wrappers around the walker (<rule>_vec, <rule>_scalar: the names profiles and tools know them by), and its entry point
// launches them through launch_stream, the one place that chooses between them.  Roofline = HBM (8 .. 32 B per element).
#include <cfloat>
#include <cstdint>
#include <type_traits>

#include "common.h"

using namespace cnn_amd;

namespace {

constexpr int kBlock = 256;

// ---- the shape ------------------------------------------------------------------------------------------------------------------------
template <bool kVec, class Op>
__device__ __forceinline__ void stream_walk(Op& op, size_t begin, size_t n) {
    const size_t lane = (size_t)blockIdx.x * kBlock + threadIdx.x, stride = (size_t)gridDim.x * kBlock;
    if constexpr (kVec) {
        const size_t n4 = n / 4;
        if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) op.template run<float>(n4 * 4 + threadIdx.x);
        for (size_t i = lane; i < n4; i += stride) op.template run<float4>(i);
    } else {
        for (size_t i = begin + lane; i < n; i += stride) op.template run<float>(i);
    }
}

// index i of a stream taken as V
template <class V>
__device__ __forceinline__ V& at(float* p, size_t i) { return reinterpret_cast<V*>(p)[i]; }
template <class V>
__device__ __forceinline__ const V& at(const float* p, size_t i) { return reinterpret_cast<const V*>(p)[i]; }

// f(values of one element ...) on the element (V = float) or on x, y, z, w in that order (V = float4); each_bit: with bit j of
// `bits` behind the j-th element's values
template <class V, class F, class... A>
__device__ __forceinline__ void each(const F& f, A&... a) {
    if constexpr (std::is_same<V, float>::value) {
        f(a...);
    } else {
        f(a.x...); f(a.y...); f(a.z...); f(a.w...);
    }
}
template <class V, class F, class... A>
__device__ __forceinline__ void each_bit(unsigned bits, const F& f, A&... a) {
    if constexpr (std::is_same<V, float>::value) {
        f(a..., bits & 1u);
    } else {
        f(a.x..., bits & 1u); f(a.y..., bits & 2u); f(a.z..., bits & 4u); f(a.w..., bits & 8u);
    }
}

// ---- ReLU -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float relu_f(float v) { return v >= 0.f ? v : 0.f; }        // relu.cpp:25
__device__ __forceinline__ float relu_b(float y, float d) { return y <= 0.f ? 0.f : d; }  // relu.cpp:38

struct ReluFwdOp {
    const float* x;
    float* y;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        V v = at<V>(x, i);
        each<V>([](float& ve) { ve = relu_f(ve); }, v);
        at<V>(y, i) = v;
    }
};
struct ReluBwdOp {
    const float* y;
    float* d;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        const V yv = at<V>(y, i);
        V dv = at<V>(d, i);
        each<V>([](float ye, float& de) { de = relu_b(ye, de); }, yv, dv);
        at<V>(d, i) = dv;
    }
};
__global__ __launch_bounds__(kBlock) void relu_fwd_vec(const ReluFwdOp op, size_t n) { stream_walk<true>(op, 0, n); }
__global__ __launch_bounds__(kBlock) void relu_fwd_scalar(const ReluFwdOp op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }
__global__ __launch_bounds__(kBlock) void relu_bwd_vec(const ReluBwdOp op, size_t n) { stream_walk<true>(op, 0, n); }
__global__ __launch_bounds__(kBlock) void relu_bwd_scalar(const ReluBwdOp op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }

// Dropout (cpu/src/dropout.cpp): CHANNEL dropout -- the first `dropped` channels of every sample are zeroed in training
// (:34-41: the loop tests the channel INDEX o against selected_num; the shuffled `sequence` only feeds the mask bookkeeping,
// so the dropped set is always channels 0 .. selected_num-1), the whole tensor is scaled by 1 - p under no_grad (:44-53).
// backward (:57-69) zeroes the same channels of the delta in place.  The scalar form only: the channel comes from the element index.
struct DropoutFwdOp {
    const float* x;
    float* y;
    int C, area, dropped, training;
    float keep;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        const int o = (int)((i / (size_t)area) % (size_t)C);
        const float v = x[i];
        y[i] = training ? (o >= dropped ? v : 0.f) : v * keep;
    }
};
struct DropoutBwdOp {
    float* d;
    int C, area, dropped;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        const int o = (int)((i / (size_t)area) % (size_t)C);
        if (o < dropped) d[i] = 0.f;
    }
};
__global__ __launch_bounds__(kBlock) void dropout_fwd(const DropoutFwdOp op, size_t n) { stream_walk<false>(op, 0, n); }
__global__ __launch_bounds__(kBlock) void dropout_bwd(const DropoutBwdOp op, size_t n) { stream_walk<false>(op, 0, n); }

// ---- the SGD step (cnn_sgd_update_keep; sgd_one(): common.h) --------------------------------------------------------------------------
// `keep` (nullable, wave-uniform): receives the value every parameter had BEFORE the step
struct SgdOp {
    float* p;
    const float* g;
    float* keep;
    float lr, scale;
    bool scaled;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        V pv = at<V>(p, i);
        const V gv = at<V>(g, i);
        if (keep) at<V>(keep, i) = pv;
        each<V>([&](float& pe, float ge) { pe = sgd_one(pe, ge, lr, scale, scaled); }, pv, gv);
        at<V>(p, i) = pv;
    }
};
__global__ __launch_bounds__(kBlock) void sgd_vec(const SgdOp op, size_t n) { stream_walk<true>(op, 0, n); }
__global__ __launch_bounds__(kBlock) void sgd_scalar(const SgdOp op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }

// ---- gradient accumulation over micro-batches (cnn_grad_accumulate) ----------------------------------------------------------------
// kFirst opens a window: acc = g, loads and stores only (every bit pattern survives, acc is not read: 8 B per element); otherwise
// acc = acc + g, one fp32 add per element (12 B per element).
template <bool kFirst>
struct GaccOp {
    float* acc;
    const float* g;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        const V gv = at<V>(g, i);
        if (kFirst) {
            at<V>(acc, i) = gv;
        } else {
            V av = at<V>(acc, i);
            each<V>([](float& ae, float ge) { ae = ae + ge; }, av, gv);
            at<V>(acc, i) = av;
        }
    }
};
template <bool kFirst>
__global__ __launch_bounds__(kBlock) void gacc_vec(const GaccOp<kFirst> op, size_t n) { stream_walk<true>(op, 0, n); }
template <bool kFirst>
__global__ __launch_bounds__(kBlock) void gacc_scalar(const GaccOp<kFirst> op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }

// ---- index ranges of the flat arena (weight decay of sgdm / adam, the averaged elements of ema) -------------------------------------
// The sorted, disjoint index ranges [begin(k), end(k)) of `r`: by value in the kernel arguments up to CNN_SGD_INLINE_RANGES of them,
// a device table beyond.  A wave's 64 float4 are 256 consecutive elements: ONE wave-uniform binary search finds the first range that
// ends behind the wave's first element; a wave that lies wholly inside or outside a range (nearly all of them: ranges are layers'
// weight blocks) is done with that, the others walk on from there per lane.
struct InlineRanges {
    uint32_t be[2 * CNN_SGD_INLINE_RANGES];
    __device__ __forceinline__ uint32_t begin(int k) const { return be[2 * k]; }
    __device__ __forceinline__ uint32_t end(int k) const { return be[2 * k + 1]; }
};
struct DeviceRanges {
    // (the constant address space: nothing writes the table while a kernel runs, so the wave-uniform search reads it with scalar loads
    // whatever the streams' pointers may alias)
    using Table = const __attribute__((address_space(4))) uint32_t*;
    Table be;
    __device__ __forceinline__ uint32_t begin(int k) const { return be[2 * k]; }
    __device__ __forceinline__ uint32_t end(int k) const { return be[2 * k + 1]; }
};
// first range that ends behind element idx (nr: none)
template <class Ranges>
__device__ __forceinline__ int first_open_range(const Ranges& r, int nr, uint32_t idx) {
    int lo = 0, hi = nr;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r.end(mid) > idx) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
template <class Ranges>
__device__ __forceinline__ bool in_range_from(const Ranges& r, int nr, int& k, uint32_t idx) {
    while (k < nr && r.end(k) <= idx) ++k;
    return k < nr && r.begin(k) <= idx;
}

// which of the four elements of float4 i are inside a range (bit j: element 4*i + j); the search is wave-uniform, see above
template <class Ranges>
__device__ __forceinline__ unsigned decay_bits4(const Ranges& r, int nr, size_t i) {
    unsigned bits = 0;
    if (nr) {
        const uint32_t e = (uint32_t)(i * 4);
        const uint32_t wave_first = __builtin_amdgcn_readfirstlane(e);  // (lanes hold ascending i: the first active one is the lowest)
        const uint64_t wave_end = (uint64_t)wave_first + 4 * kWave;
        const int k0 = first_open_range(r, nr, wave_first);
        if (k0 < nr) {
            const uint32_t b0 = r.begin(k0);
            if (b0 <= wave_first && r.end(k0) >= wave_end) {
                bits = 15u;
            } else if (b0 < wave_end) {
                int k = k0;
#pragma unroll
                for (int j = 0; j < 4; ++j) bits |= in_range_from(r, nr, k, e + j) ? (1u << j) : 0u;
            }
        }
    }
    return bits;
}
// one element's answer (the tails and the scalar kernels)
template <class Ranges>
__device__ __forceinline__ bool decays_at(const Ranges& r, int nr, size_t i) {
    int k = nr ? first_open_range(r, nr, (uint32_t)i) : 0;
    return nr && in_range_from(r, nr, k, (uint32_t)i);
}
// the bits of index i of a stream taken as V (each_bit's).  An Op asks AFTER it has issued its streams' loads: the table search runs
// while they are in flight.
template <class V, class Ranges>
__device__ __forceinline__ unsigned range_bits(const Ranges& r, int nr, size_t i) {
    if constexpr (std::is_same<V, float>::value) return decays_at(r, nr, i) ? 1u : 0u;
    else return decay_bits4(r, nr, i);
}

// ---- SGD with momentum / weight decay / Nesterov (cnn_sgd_momentum_update; sgdm_one(): common.h) -----------------------------
// Reads p, g, v and writes p, v (20 B per element, 24 with the nullable `keep`); kMomentum = false neither reads nor writes v.  Weight
// decay applies inside the ranges of `r` only.
struct SgdmArgs {
    float lr, momentum, wd, scale;
    bool scaled, nesterov;
    int nr;  // number of ranges; 0 when weight_decay == 0
};
template <bool kMomentum, class Ranges>
struct SgdmOp {
    float* p;
    const float* g;
    float* v;
    float* keep;
    SgdmArgs a;
    Ranges r;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        V pv = at<V>(p, i);
        const V gv = at<V>(g, i);
        V vv = kMomentum ? at<V>(v, i) : V{};
        const unsigned bits = range_bits<V>(r, a.nr, i);  // bit j: the j-th element decays
        if (keep) at<V>(keep, i) = pv;
        each_bit<V>(bits, [&](float& pe, float ge, float& ve, bool decay) {
            pe = sgdm_one<kMomentum>(pe, ge, ve, a.lr, a.momentum, a.wd, a.scale, a.scaled, decay, a.nesterov);
        }, pv, gv, vv);
        at<V>(p, i) = pv;
        if (kMomentum) at<V>(v, i) = vv;
    }
};
template <bool kMomentum, class Ranges>
__global__ __launch_bounds__(kBlock) void sgdm_vec(const SgdmOp<kMomentum, Ranges> op, size_t n) { stream_walk<true>(op, 0, n); }
template <bool kMomentum, class Ranges>
__global__ __launch_bounds__(kBlock) void sgdm_scalar(const SgdmOp<kMomentum, Ranges> op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }

// ---- Adam / AdamW (cnn_adam_update; adam_one(): common.h) -------------------------------------------------------------------------
// Four streams: reads p, g, m, v and writes p, m, v (28 B per element, 32 with keep); weight decay inside the ranges of `r` only.
// Three correctly rounded divide / root sequences per element.
struct AdamArgs {
    AdamScalars s;
    int nr;  // number of ranges; 0 when weight_decay == 0
};
template <class Ranges>
struct AdamOp {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* keep;
    AdamArgs a;
    Ranges r;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        V pv = at<V>(p, i);
        const V gv = at<V>(g, i);
        V mv = at<V>(m, i);
        V vv = at<V>(v, i);
        const unsigned bits = range_bits<V>(r, a.nr, i);  // bit j: the j-th element decays
        if (keep) at<V>(keep, i) = pv;
        each_bit<V>(bits, [&](float& pe, float ge, float& me, float& ve, bool decay) { pe = adam_one(pe, ge, me, ve, a.s, decay); }, pv, gv, mv, vv);
        at<V>(p, i) = pv;
        at<V>(m, i) = mv;
        at<V>(v, i) = vv;
    }
};
template <class Ranges>
__global__ __launch_bounds__(kBlock) void adam_vec(const AdamOp<Ranges> op, size_t n) { stream_walk<true>(op, 0, n); }
template <class Ranges>
__global__ __launch_bounds__(kBlock) void adam_scalar(const AdamOp<Ranges> op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }

// ---- exponential moving average of the parameters (cnn_ema_update) ----------------------------------------------------------------
// Reads ema, p and writes ema (12 B per element).  The ranges of `r` are the elements that are AVERAGED (ema = decay * ema + omd * p,
// two products and one sum, each rounded); the others -- BatchNorm2D's moving statistics -- take p's bits.  decay == 0 or an empty
// table averages nothing: that call is GaccOp<true> (acc = g: loads and stores only, ema is not read, 8 B per element) under the
// names ema_vec_copy / ema_scalar_copy.
struct EmaArgs {
    float decay, omd;
    int nr;  // number of ranges, >= 1
};
__device__ __forceinline__ float ema_one(float e, float p, float decay, float omd, bool averaged) {
#pragma clang fp contract(off)
    const float de = decay * e;
    const float op = omd * p;
    const float sum = de + op;
    return averaged ? sum : p;  // (a select: p's bits as they are)
}
template <class Ranges>
struct EmaOp {
    float* ema;
    const float* p;
    EmaArgs a;
    Ranges r;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        V ev = at<V>(ema, i);
        const V pv = at<V>(p, i);
        const unsigned bits = range_bits<V>(r, a.nr, i);  // bit j: the j-th element is averaged
        each_bit<V>(bits, [&](float& ee, float pe, bool averaged) { ee = ema_one(ee, pe, a.decay, a.omd, averaged); }, ev, pv);
        at<V>(ema, i) = ev;
    }
};
template <class Ranges>
__global__ __launch_bounds__(kBlock) void ema_vec(const EmaOp<Ranges> op, size_t n) { stream_walk<true>(op, 0, n); }
template <class Ranges>
__global__ __launch_bounds__(kBlock) void ema_scalar(const EmaOp<Ranges> op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }

// ---- exchange of two disjoint buffers (cnn_arena_swap) -------------------------------------------------------------------------------
// Loads and stores only, every bit pattern survives; reads and writes both (16 B per element).  The buffers do not overlap (checked
// by the entry), so every element is read before either copy of it is written.
struct SwapOp {
    float* a;
    float* b;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        const V av = at<V>(a, i);
        const V bv = at<V>(b, i);
        at<V>(a, i) = bv;
        at<V>(b, i) = av;
    }
};
__global__ __launch_bounds__(kBlock) void aswap_vec(const SwapOp op, size_t n) { stream_walk<true>(op, 0, n); }
__global__ __launch_bounds__(kBlock) void aswap_scalar(const SwapOp op, size_t begin, size_t n) { stream_walk<false>(op, begin, n); }

// ---- clipping by the global L2 norm (cnn_clip_grad_norm) ----------------------------------------------------------------------------
// Three launches, no host round trip, no floating-point atomics:
//   clip_partial : every workgroup sums (double)g * (double)g over its share of the walk (per lane in the walk's order -- the tail
//                  element, then x, y, z, w of each float4 --, then the wave's shuffle tree, then the four waves in order) into
//                  partial[blockIdx.x] -- the products are exact in fp64;
//   clip_finish  : ONE workgroup adds the partials (each lane its strided share in ascending order, then the same tree), takes the
//                  root, and writes stats = {total norm, coefficient};
//   clip_scale   : g *= coefficient; every workgroup returns at once when the coefficient is 1 (the arena is not written).
// The order of every sum is fixed by n and the grid alone, so the result is the same from run to run.  The grid never exceeds
// kClipMaxBlocks workgroups: the workspace is that many doubles whatever n is.
constexpr int kClipMaxBlocks = CNN_CLIP_MAX_BLOCKS;

__device__ __forceinline__ double block_sum(double x, double* lds) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x += __shfl_down(x, off, kWave);
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) lds[wave] = x;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0) {
        total = lds[0];
        for (int w = 1; w < kBlock / kWave; ++w) total += lds[w];
    }
    return total;  // (valid in thread 0)
}

struct SumSqOp {
    const float* g;
    double acc;  // the lane's sum
    template <class V>
    __device__ __forceinline__ void run(size_t i) {
        const V q = at<V>(g, i);
        each<V>([&](float ge) {
            const double x = (double)ge;
            acc += x * x;
        }, q);
    }
};
struct ScaleOp {
    float* g;
    float coef;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        V q = at<V>(g, i);
        each<V>([&](float& ge) { ge *= coef; }, q);
        at<V>(g, i) = q;
    }
};

template <bool kVec>
__global__ __launch_bounds__(kBlock) void clip_partial(const float* __restrict__ g, size_t n, double* __restrict__ partial) {
    __shared__ double lds[kBlock / kWave];
    SumSqOp op{g, 0.0};
    stream_walk<kVec>(op, 0, n);
    const double total = block_sum(op.acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void clip_finish(const double* __restrict__ partial, int n_partial, float max_norm, float scale, bool scaled,
                                                      float* __restrict__ stats) {
    __shared__ double lds[kBlock / kWave];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[i];
    const double S = block_sum(acc, lds);
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const float norm = (float)sqrt(S);
        const float total = scaled ? norm * scale : norm;
        const float sum = total + 1e-6f;
        const float c = max_norm / sum;
        stats[0] = total;
        stats[1] = c < 1.f ? c : 1.f;  // (a NaN total: the comparison is false, the gradients stay as they are)
    }
}

template <bool kVec>
__global__ __launch_bounds__(kBlock) void clip_scale(float* __restrict__ g, size_t n, const float* __restrict__ stats) {
    const float coef = stats[1];
    if (!(coef < 1.f)) return;
    const ScaleOp op{g, coef};
    stream_walk<kVec>(op, 0, n);
}

// One workgroup; thread t owns samples t, t+256, ...  Per-sample arithmetic is the reference's sequential
// loop (func.cpp:22-33, 63-68); the loss terms are then added in ascending sample order by one lane so the
// fp32 loss sum has the reference's order (func.cpp:60-71).
// SOFT (cnn_softmax_xent_soft): `labels` is a dense [B][classes] fp32 target tensor, yv = targets[b][i]; the same expressions otherwise.
template <bool SOFT>
__global__ __launch_bounds__(kBlock) void softmax_xent_kernel(const float* __restrict__ logits,
                                                              const std::conditional_t<SOFT, float, int32_t>* __restrict__ labels,
                                                              float* __restrict__ probs, float* __restrict__ delta,
                                                              float* __restrict__ loss_sum, int B, int classes) {
    __shared__ float terms[kBlock];
    float running = 0.f;
    for (int base = 0; base < B; base += kBlock) {
        const int b = base + threadIdx.x;
        float term = 0.f;
        if (b < B) {
            const float* in = logits + (size_t)b * classes;
            float mx = in[0];  // Tensor3D::max = first maximum, strict '>' (data_format.cpp:37-48)
            for (int i = 1; i < classes; ++i)
                if (in[i] > mx) mx = in[i];
            float sum = 0.f;
            for (int i = 0; i < classes; ++i) sum += clamped_exp(in[i] - mx);
            int label = 0;
            if constexpr (!SOFT) label = labels[b];
            for (int i = 0; i < classes; ++i) {
                float p = clamped_exp(in[i] - mx) / sum;
                if (isnan(p)) p = 0.f;
                float yv;
                if constexpr (SOFT) yv = labels[(size_t)b * classes + i];
                else yv = (i == label) ? 1.f : 0.f;
                if (probs) probs[(size_t)b * classes + i] = p;
                delta[(size_t)b * classes + i] = p - yv;  // no 1/B here (func.cpp:64)
                term += logf(p) * yv;                     // func.cpp:65, incl. its log(0)*0 = NaN behaviour
            }
        }
        terms[threadIdx.x] = term;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(kBlock, B - base);
            for (int i = 0; i < cnt; ++i) running += terms[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && loss_sum) loss_sum[0] = -running;
}

// ---- soft targets from labels (cnn_soft_targets) --------------------------------------------------------------------------------------
// the partner of sample b under a pair rule (include/cnn_amd.h); `rule` is never CNN_PAIR_NONE here
__device__ __forceinline__ int pair_of(int b, int B, int rule, int shift) {
    if (rule == CNN_PAIR_FLIP) return B - 1 - b;
    const int p = b + (shift - B);  // (b + shift) % B without the division: 1 <= shift < B
    return p < 0 ? p + B : p;
}
struct SoftTargetArgs {
    int B, classes, rule, shift;
    float u, hot, lam, oml;  // u = smoothing / classes, hot = (1 - smoothing) + u, oml = 1 - lam: the host's fp32 values
    bool smooth;             // smoothing != 0
};
// A lane per target value: t[b][j] = base(labels[b], j), or lam * base(labels[b], j) + oml * base(labels[p(b)], j) -- two products and one
// sum, each rounded.  A label outside [0, classes) matches no j.
__global__ __launch_bounds__(kBlock) void soft_targets_kernel(const int32_t* __restrict__ labels, float* __restrict__ targets, const SoftTargetArgs a) {
#pragma clang fp contract(off)
    const size_t n = (size_t)a.B * a.classes, stride = (size_t)gridDim.x * kBlock;
    for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        const int b = (int)(e / (size_t)a.classes), j = (int)(e - (size_t)b * a.classes);
        const auto base = [&](int label) { return a.smooth ? (j == label ? a.hot : a.u) : (j == label ? 1.f : 0.f); };
        const float own = base(labels[b]);
        if (a.rule == CNN_PAIR_NONE) {
            targets[e] = own;
        } else {
            const float other = base(labels[pair_of(b, a.B, a.rule, a.shift)]);
            const float po = a.lam * own;
            const float pp = a.oml * other;
            targets[e] = po + pp;
        }
    }
}

// ---- mixup / CutMix of a batch with its partner samples (cnn_batch_mix) ---------------------------------------------------------------
// Out of place: dst[b] from src[b] and src[p(b)].  The grid's rows walk the samples, so the partner is uniform in a workgroup and costs
// no per-element division; inside a sample the columns of the grid run stream_walk over its C*H*W elements -- the float4 form when
// every sample starts 16-byte aligned (both pointers aligned, C*H*W % 4 == 0), the scalar form otherwise.
struct BmixArgs {
    size_t ns;  // elements per sample
    int B, rule, shift;
};
__device__ __forceinline__ float mix_one(float a, float p, float lam, float oml) {
#pragma clang fp contract(off)
    const float la = lam * a;
    const float op = oml * p;
    return la + op;
}
// mixup: reads the sample and its partner, writes the mix (12 B per element)
struct MixupOp {
    const float* own;
    const float* partner;
    float* out;
    float lam, oml;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        V av = at<V>(own, i);
        const V pv = at<V>(partner, i);
        each<V>([&](float& ae, float pe) { ae = mix_one(ae, pe, lam, oml); }, av, pv);
        at<V>(out, i) = av;
    }
};
// CutMix: a copy of the bits, from the partner inside the box and from the sample outside (8 B per element: a float4 that lies wholly
// inside or outside requests one of the two lines, only one that the box's edge cuts requests both).  Row and column of an element come
// from two 32-bit divisions per float4 (or per element in the scalar form); a float4 that runs over the end of its row (W % 4 != 0) takes
// them per element.
struct CutBox {
    uint32_t H, W, y0, y1, x0, x1;
    __device__ __forceinline__ bool holds(uint32_t e) const {
        const uint32_t row = e / W, x = e - row * W, y = row % H;
        return y >= y0 && y < y1 && x >= x0 && x < x1;
    }
};
struct CutmixOp {
    const float* own;
    const float* partner;
    float* out;
    CutBox box;
    template <class V>
    __device__ __forceinline__ void run(size_t i) const {
        if constexpr (std::is_same<V, float>::value) {
            at<V>(out, i) = box.holds((uint32_t)i) ? partner[i] : own[i];
        } else {
            const uint32_t e = (uint32_t)i * 4u;
            const uint32_t row = e / box.W, x = e - row * box.W, y = row % box.H;
            unsigned bits = 0;
            if (x + 3 < box.W) {  // the four elements share a row
                if (y >= box.y0 && y < box.y1)
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) bits |= (x + j >= box.x0 && x + j < box.x1) ? (1u << j) : 0u;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) bits |= box.holds(e + j) ? (1u << j) : 0u;
            }
            V v;
            if (bits == 0u) {
                v = at<V>(own, i);
            } else if (bits == 15u) {
                v = at<V>(partner, i);
            } else {
                v = at<V>(own, i);
                const V pv = at<V>(partner, i);
                each_bit<V>(bits, [](float& ve, float pe, bool inside) { ve = inside ? pe : ve; }, v, pv);
            }
            at<V>(out, i) = v;
        }
    }
};
template <bool kVec>
__global__ __launch_bounds__(kBlock) void bmix_mixup(const float* __restrict__ src, float* __restrict__ dst, const BmixArgs a, float lam, float oml) {
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const MixupOp op{src + (size_t)b * a.ns, src + (size_t)pair_of(b, a.B, a.rule, a.shift) * a.ns, dst + (size_t)b * a.ns, lam, oml};
        stream_walk<kVec>(op, 0, a.ns);
    }
}
template <bool kVec>
__global__ __launch_bounds__(kBlock) void bmix_cutmix(const float* __restrict__ src, float* __restrict__ dst, const BmixArgs a, const CutBox box) {
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const CutmixOp op{src + (size_t)b * a.ns, src + (size_t)pair_of(b, a.B, a.rule, a.shift) * a.ns, dst + (size_t)b * a.ns, box};
        stream_walk<kVec>(op, 0, a.ns);
    }
}

// ---- host side: the one launcher of the streaming shape -----------------------------------------------------------------------------
// Which launches an entry makes over n elements, and how the launch log shows them:
//   kTailRides : ONE launch -- the float4 kernel over all n (the n % 4 trailing elements ride in its workgroup 0) when every pointer
//                is 16-byte aligned and n >= 4, the scalar kernel alone otherwise;
//   kSplit     : the float4 kernel over n / 4 * 4 elements under the same condition, then the scalar kernel over the rest (ReLU);
//   kClip      : kTailRides on clip_grid, the float4 kernel whatever n is, no "tail" in the scalar kernel's geometry (the clip passes).
// vec(grid, n_vec) / scalar(grid, begin) launch and return nothing.  The geometry is "n=<n>" for the float4 kernel and "tail n=<what
// the scalar kernel covers>" for the other, with " ranges=<nr>" behind it where nr >= 0.
enum StreamForm { kTailRides, kSplit, kClip };

// grid of the clip kernels: stream_grid, never more than the workspace holds
inline unsigned clip_grid(size_t work_items) {
    const unsigned g = stream_grid(work_items, kBlock);
    return g > (unsigned)kClipMaxBlocks ? (unsigned)kClipMaxBlocks : g;
}

template <class Vec, class Scalar>
int launch_stream(hipStream_t s, const char* vec_name, const char* scalar_name, StreamForm form, bool all_aligned, size_t n, int nr,
                  const Vec& vec, const Scalar& scalar) {
    const auto grid = [&](size_t work_items) { return form == kClip ? clip_grid(work_items) : stream_grid(work_items, kBlock); };
    size_t begin = 0;
    if (all_aligned && (n >= 4 || form == kClip)) {
        begin = form == kSplit ? n / 4 * 4 : n;
        CNN_KLAUNCH(s, vec_name, vec(grid(n / 4), begin), nr < 0 ? "n=%zu" : "n=%zu ranges=%d", n, nr);
    }
    if (begin < n) {
        const char* tag = form == kClip ? "n=%zu" : nr < 0 ? "tail n=%zu" : "tail n=%zu ranges=%d";
        CNN_KLAUNCH(s, scalar_name, scalar(grid(n - begin), begin), tag, n - begin, nr);
    }
    return CNN_AMD_OK;
}
// ... of an Op and its two wrappers
template <class Op>
int launch_stream(hipStream_t s, const char* vec_name, void (*vec)(Op, size_t), const char* scalar_name, void (*scalar)(Op, size_t, size_t),
                  StreamForm form, bool all_aligned, size_t n, int nr, const Op& op) {
    return launch_stream(
        s, vec_name, scalar_name, form, all_aligned, n, nr, [&](unsigned grid, size_t n_vec) { vec<<<grid, kBlock, 0, s>>>(op, n_vec); },
        [&](unsigned grid, size_t begin) { scalar<<<grid, kBlock, 0, s>>>(op, begin, n); });
}

// ---- host side shared by the arena entries with a range table (cnn_sgd_momentum_update, cnn_adam_update, cnn_ema_update) ---------------
// the range table of an entry: n fits the 32-bit table, the ranges are there, sorted, disjoint, non-empty and inside [0, n)
int check_decay_ranges(const char* entry, size_t n, const uint32_t* decay_ranges, const uint32_t* decay_ranges_dev, size_t n_ranges) {
    CNN_REQUIRE(n <= (size_t)0xFFFFFFFFu - 4 * kWave, "%s: n=%zu exceeds the 32-bit range table: step the arena in pieces", entry, n);
    CNN_REQUIRE(n_ranges <= n && (n_ranges == 0 || decay_ranges), "%s: null decay_ranges / n_ranges=%zu with n=%zu", entry, n_ranges, n);
    CNN_REQUIRE(n_ranges <= (size_t)CNN_SGD_INLINE_RANGES || decay_ranges_dev, "%s: %zu ranges (more than CNN_SGD_INLINE_RANGES) need decay_ranges_dev",
                entry, n_ranges);
    uint32_t prev_end = 0;
    for (size_t k = 0; k < n_ranges; ++k) {
        const uint32_t b = decay_ranges[2 * k], e = decay_ranges[2 * k + 1];
        CNN_REQUIRE(b >= prev_end && b < e && (size_t)e <= n, "%s: range %zu = [%u, %u) is empty, unsorted, overlapping or beyond n=%zu", entry, k, b, e, n);
        prev_end = e;
    }
    return CNN_AMD_OK;
}

// calls launch(ranges) with the first nr ranges by value in the kernel arguments, or with the device table beyond CNN_SGD_INLINE_RANGES
template <class Launch>
int with_ranges(int nr, const uint32_t* decay_ranges, const uint32_t* decay_ranges_dev, const Launch& launch) {
    if (nr > CNN_SGD_INLINE_RANGES) return launch(DeviceRanges{(DeviceRanges::Table)decay_ranges_dev});
    InlineRanges r;
    for (int k = 0; k < 2 * CNN_SGD_INLINE_RANGES; ++k) r.be[k] = k < 2 * nr ? decay_ranges[k] : 0u;
    return launch(r);
}

template <bool kMomentum, class Ranges>
int launch_sgdm(float* params, const float* grads, float* velocity, size_t n, const SgdmArgs& a, float* previous, const Ranges& r,
                hipStream_t s) {
    const bool aligned = aligned16(params) && aligned16(grads) && (!kMomentum || aligned16(velocity)) && (previous == nullptr || aligned16(previous));
    return launch_stream(s, "sgdm_vec", sgdm_vec<kMomentum, Ranges>, "sgdm_scalar", sgdm_scalar<kMomentum, Ranges>, kTailRides, aligned, n, a.nr,
                         SgdmOp<kMomentum, Ranges>{params, grads, velocity, previous, a, r});
}

// the scalars of one Adam step that do not depend on the element (common.h, adam_one): plain host arithmetic, every fp32 operation
// rounded separately
AdamScalars adam_scalars(const cnn_adam_options& o, float grad_scale) {
#pragma clang fp contract(off)
    AdamScalars a;
    a.beta1 = o.beta1;
    a.beta2 = o.beta2;
    a.omb1 = 1.f - o.beta1;
    a.omb2 = 1.f - o.beta2;
    a.eps = o.eps;
    a.wd = o.weight_decay;
    const volatile float lw = o.lr * o.weight_decay;
    a.om = 1.f - lw;
    const double t = (double)o.step;
    a.bc2s = (float)std::sqrt(1.0 - std::pow((double)o.beta2, t));
    a.ss = (float)((double)o.lr / (1.0 - std::pow((double)o.beta1, t)));
    a.scale = grad_scale;
    a.scaled = grad_scale != 1.0f;
    a.decoupled = o.decoupled != 0;
    return a;
}

// ---- AlexNet::grad_cam (alexnet.cpp:107-140) on a [B][C][H][W] feature map -------------------------------------------------
// weights[b][o] = (sum_i fea[b][o][i]) / area, sequential in i (:111-119; the reference takes the channel mean of the FEATURE MAP,
// not of a gradient); cam[b][i] = sum_o weights[b][o] * fea[b][o][i], sequential in o, multiply-then-add (:124-131); ReLU as
// `if (v < 0) v = 0` (:134).  One workgroup per sample: thread t owns channels t, t+256, ... in the first phase, pixels in the second.
__global__ __launch_bounds__(kBlock) void grad_cam_maps(const float* __restrict__ fea, float* __restrict__ cam, int C, int area) {
    extern __shared__ float wts[];
    const float* fb = fea + (size_t)blockIdx.x * C * area;
    for (int o = threadIdx.x; o < C; o += kBlock) {
        const float* f = fb + (size_t)o * area;
        float m = 0.f;
        for (int i = 0; i < area; ++i) m += f[i];
        wts[o] = m / area;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < area; i += kBlock) {
#pragma clang fp contract(off)
        float acc = 0.f;
        for (int o = 0; o < C; ++o) {
            const float prod = wts[o] * fb[(size_t)o * area + i];
            acc = acc + prod;
        }
        if (acc < 0.f) acc = 0.f;
        cam[(size_t)blockIdx.x * area + i] = acc;
    }
}
// min-max normalisation over the WHOLE [B][H][W] tensor (:136-139; Tensor3D::min/max = first extremum with strict comparisons,
// data_format.cpp:37-62: a NaN is only ever returned from element 0) and the 8-bit image of the first plane (opecv_mat(1),
// data_format.cpp:98-103: saturate_cast<uchar>(255 * v) = round to nearest even, clamped)
__global__ __launch_bounds__(kBlock) void grad_cam_normalise(float* __restrict__ cam, unsigned char* __restrict__ image, size_t n, int area) {
    __shared__ float smin[kBlock], smax[kBlock];
    const float first = cam[0];
    float lo = INFINITY, hi = -INFINITY;
    for (size_t i = threadIdx.x; i < n; i += kBlock) {
        const float v = cam[i];
        if (v < lo) lo = v;
        if (v > hi) hi = v;
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            if (smin[threadIdx.x + off] < smin[threadIdx.x]) smin[threadIdx.x] = smin[threadIdx.x + off];
            if (smax[threadIdx.x + off] > smax[threadIdx.x]) smax[threadIdx.x] = smax[threadIdx.x + off];
        }
        __syncthreads();
    }
    // element 0 is the start value of both scans: a NaN there survives every comparison; all-NaN tails leave +-inf, which the
    // reference cannot produce (it starts from element 0) -- fall back to element 0 then
    float mn = smin[0], mx = smax[0];
    if (first != first) mn = mx = first;
    else {
        if (!(mn <= first)) mn = first;
        if (!(mx >= first)) mx = first;
    }
    const float res = mx - mn;
    __syncthreads();
    for (size_t i = threadIdx.x; i < n; i += kBlock) {
        const float v = (cam[i] - mn) / res;
        cam[i] = v;
        if (image && i < (size_t)area) {
            const float sv = 255.f * v;
            int r = (sv != sv) ? 0 : (sv >= 255.5f ? 255 : (sv <= -0.5f ? 0 : __float2int_rn(sv)));
            image[i] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
        }
    }
}

}  // namespace

extern "C" {

int cnn_relu_forward(const float* x, float* y, size_t n, void* stream) {
    if (n == 0) return CNN_AMD_OK;
    CNN_REQUIRE(x && y, "cnn_relu_forward: null pointer");
    return launch_stream(as_stream(stream), "relu_fwd_vec", relu_fwd_vec, "relu_fwd_scalar", relu_fwd_scalar, kSplit, aligned16(x) && aligned16(y), n, -1,
                         ReluFwdOp{x, y});
}

int cnn_relu_backward(const float* y, float* dy, size_t n, void* stream) {
    if (n == 0) return CNN_AMD_OK;
    CNN_REQUIRE(y && dy, "cnn_relu_backward: null pointer");
    return launch_stream(as_stream(stream), "relu_bwd_vec", relu_bwd_vec, "relu_bwd_scalar", relu_bwd_scalar, kSplit, aligned16(y) && aligned16(dy), n, -1,
                         ReluBwdOp{y, dy});
}

int cnn_sgd_update(float* params, const float* grads, size_t n, float lr, float grad_scale, void* stream) {
    return cnn_sgd_update_keep(params, grads, n, lr, grad_scale, nullptr, stream);
}

int cnn_sgd_update_keep(float* params, const float* grads, size_t n, float lr, float grad_scale, float* previous, void* stream) {
    if (n == 0) return CNN_AMD_OK;
    CNN_REQUIRE(params && grads, "cnn_sgd_update: null pointer");
    const bool aligned = aligned16(params) && aligned16(grads) && (previous == nullptr || aligned16(previous));
    return launch_stream(as_stream(stream), "sgd_vec", sgd_vec, "sgd_scalar", sgd_scalar, kTailRides, aligned, n, -1,
                         SgdOp{params, grads, previous, lr, grad_scale, grad_scale != 1.0f});
}

int cnn_grad_accumulate(float* acc, const float* grads, size_t n, int first, void* stream) {
    CNN_REQUIRE(acc && grads, "cnn_grad_accumulate: null pointer");
    CNN_REQUIRE(n != 0, "cnn_grad_accumulate: n=0");
    CNN_REQUIRE(acc != grads, "cnn_grad_accumulate: acc and grads are the same buffer");
    hipStream_t s = as_stream(stream);
    const bool aligned = aligned16(acc) && aligned16(grads);
    return first ? launch_stream(s, "gacc_vec_first", gacc_vec<true>, "gacc_scalar_first", gacc_scalar<true>, kTailRides, aligned, n, -1, GaccOp<true>{acc, grads})
                 : launch_stream(s, "gacc_vec_add", gacc_vec<false>, "gacc_scalar_add", gacc_scalar<false>, kTailRides, aligned, n, -1, GaccOp<false>{acc, grads});
}

float cnn_ema_decay_at(float decay, int warmup, uint64_t updates_done) {
    if (warmup == 0) return decay;
    const double t = (double)updates_done;
    const float ramp = (float)((1.0 + t) / (10.0 + t));
    return ramp < decay ? ramp : decay;
}

// two runs of n floats share an element
static bool floats_overlap(const float* a, const float* b, size_t n) {
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
    return (ua > ub ? ua - ub : ub - ua) < (uintptr_t)n * sizeof(float);
}

int cnn_ema_update(float* ema, const float* params, size_t n, float decay, const uint32_t* avg_ranges, const uint32_t* avg_ranges_dev,
                   size_t n_ranges, void* stream) {
    CNN_REQUIRE(ema && params, "cnn_ema_update: null pointer");
    CNN_REQUIRE(n != 0, "cnn_ema_update: n=0");
    CNN_REQUIRE(!floats_overlap(ema, params, n), "cnn_ema_update: ema and params are the same buffer or overlap");
    CNN_REQUIRE(decay >= 0.f && decay < 1.f, "cnn_ema_update: decay=%g outside [0, 1)", (double)decay);
    if (int rc = check_decay_ranges("cnn_ema_update", n, avg_ranges, avg_ranges_dev, n_ranges)) return rc;
    hipStream_t s = as_stream(stream);
    const bool aligned = aligned16(ema) && aligned16(params);
    if (decay == 0.f || n_ranges == 0)  // nothing is averaged: the copy of the bits
        return launch_stream(s, "ema_vec_copy", gacc_vec<true>, "ema_scalar_copy", gacc_scalar<true>, kTailRides, aligned, n, 0, GaccOp<true>{ema, params});
    EmaArgs a;
    a.decay = decay;
    a.omd = 1.f - decay;
    a.nr = (int)n_ranges;
    return with_ranges(a.nr, avg_ranges, avg_ranges_dev, [&](const auto& r) {
        using Ranges = std::decay_t<decltype(r)>;
        return launch_stream(s, "ema_vec", ema_vec<Ranges>, "ema_scalar", ema_scalar<Ranges>, kTailRides, aligned, n, a.nr, EmaOp<Ranges>{ema, params, a, r});
    });
}

int cnn_arena_swap(float* a, float* b, size_t n, void* stream) {
    CNN_REQUIRE(a && b, "cnn_arena_swap: null pointer");
    CNN_REQUIRE(n != 0, "cnn_arena_swap: n=0");
    CNN_REQUIRE(!floats_overlap(a, b, n), "cnn_arena_swap: a and b are the same buffer or overlap");
    return launch_stream(as_stream(stream), "aswap_vec", aswap_vec, "aswap_scalar", aswap_scalar, kTailRides, aligned16(a) && aligned16(b), n, 0, SwapOp{a, b});
}

// (the two update entries differ in when n == 0 returns: this one returns OK before it looks at any argument, cnn_adam_update validates
// its arguments first.  Both orders are what the entries have always done; callers may rely on either.)
int cnn_sgd_momentum_update(float* params, const float* grads, float* velocity, size_t n, const cnn_sgd_options* opt, float grad_scale,
                            const uint32_t* decay_ranges, const uint32_t* decay_ranges_dev, size_t n_ranges, float* previous,
                            void* stream) {
    if (n == 0) return CNN_AMD_OK;
    CNN_REQUIRE(params && grads && opt, "cnn_sgd_momentum_update: null pointer");
    CNN_REQUIRE(opt->momentum >= 0.f && opt->weight_decay >= 0.f, "cnn_sgd_momentum_update: momentum=%g weight_decay=%g", (double)opt->momentum,
                (double)opt->weight_decay);
    CNN_REQUIRE(velocity || opt->momentum == 0.f, "cnn_sgd_momentum_update: null velocity with momentum=%g", (double)opt->momentum);
    if (int rc = check_decay_ranges("cnn_sgd_momentum_update", n, decay_ranges, decay_ranges_dev, n_ranges)) return rc;
    hipStream_t s = as_stream(stream);
    SgdmArgs a;
    a.lr = opt->lr;
    a.momentum = opt->momentum;
    a.wd = opt->weight_decay;
    a.scale = grad_scale;
    a.scaled = grad_scale != 1.0f;
    a.nesterov = opt->nesterov != 0;
    a.nr = opt->weight_decay != 0.f ? (int)n_ranges : 0;
    const bool mom = opt->momentum != 0.f;
    return with_ranges(a.nr, decay_ranges, decay_ranges_dev, [&](const auto& r) {
        return mom ? launch_sgdm<true>(params, grads, velocity, n, a, previous, r, s) : launch_sgdm<false>(params, grads, velocity, n, a, previous, r, s);
    });
}

int cnn_adam_update(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, const cnn_adam_options* opt,
                    float grad_scale, const uint32_t* decay_ranges, const uint32_t* decay_ranges_dev, size_t n_ranges, float* previous,
                    void* stream) {
    CNN_REQUIRE(params && grads && exp_avg && exp_avg_sq && opt, "cnn_adam_update: null pointer");
    CNN_REQUIRE(opt->beta1 >= 0.f && opt->beta1 < 1.f && opt->beta2 >= 0.f && opt->beta2 < 1.f, "cnn_adam_update: beta1=%g beta2=%g outside [0, 1)",
                (double)opt->beta1, (double)opt->beta2);
    CNN_REQUIRE(opt->eps > 0.f, "cnn_adam_update: eps=%g must be positive", (double)opt->eps);
    CNN_REQUIRE(opt->weight_decay >= 0.f, "cnn_adam_update: weight_decay=%g", (double)opt->weight_decay);
    CNN_REQUIRE(opt->step != 0, "cnn_adam_update: step=0 (the number of this step, counted from 1)");
    if (int rc = check_decay_ranges("cnn_adam_update", n, decay_ranges, decay_ranges_dev, n_ranges)) return rc;
    if (n == 0) return CNN_AMD_OK;
    hipStream_t s = as_stream(stream);
    AdamArgs a;
    a.s = adam_scalars(*opt, grad_scale);
    a.nr = opt->weight_decay != 0.f ? (int)n_ranges : 0;
    const bool aligned = aligned16(params) && aligned16(grads) && aligned16(exp_avg) && aligned16(exp_avg_sq) && (previous == nullptr || aligned16(previous));
    return with_ranges(a.nr, decay_ranges, decay_ranges_dev, [&](const auto& r) {
        using Ranges = std::decay_t<decltype(r)>;
        return launch_stream(s, "adam_vec", adam_vec<Ranges>, "adam_scalar", adam_scalar<Ranges>, kTailRides, aligned, n, a.nr,
                             AdamOp<Ranges>{params, grads, exp_avg, exp_avg_sq, previous, a, r});
    });
}

size_t cnn_clip_grad_norm_workspace_bytes(size_t n) {
    // one double per workgroup of the largest grid a call with this n launches (the scalar kernels': one element per lane)
    const size_t need = (n + kBlock - 1) / kBlock;
    return sizeof(double) * (need < 1 ? 1 : (need > (size_t)kClipMaxBlocks ? (size_t)kClipMaxBlocks : need));
}

int cnn_clip_grad_norm(float* grads, size_t n, float max_norm, float grad_scale, void* workspace, size_t workspace_bytes, float* stats_dev,
                       void* stream) {
    CNN_REQUIRE(grads && workspace && stats_dev, "cnn_clip_grad_norm: null pointer");
    CNN_REQUIRE(n != 0, "cnn_clip_grad_norm: n=0");
    CNN_REQUIRE(max_norm > 0.f, "cnn_clip_grad_norm: max_norm=%g must be positive", (double)max_norm);
    const size_t need = cnn_clip_grad_norm_workspace_bytes(n);
    CNN_REQUIRE(workspace_bytes >= need, "cnn_clip_grad_norm: workspace of %zu bytes, n=%zu needs %zu (cnn_clip_grad_norm_workspace_bytes)",
                workspace_bytes, n, need);
    CNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "cnn_clip_grad_norm: the workspace must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    double* partial = (double*)workspace;
    const bool aligned = aligned16(grads);
    unsigned partials = 0;  // the grid of the first pass
    if (int rc = launch_stream(
            s, "clip_partial_vec", "clip_partial_scalar", kClip, aligned, n, -1,
            [&](unsigned grid, size_t) { clip_partial<true><<<grid, kBlock, 0, s>>>(grads, n, partial), partials = grid; },
            [&](unsigned grid, size_t) { clip_partial<false><<<grid, kBlock, 0, s>>>(grads, n, partial), partials = grid; }))
        return rc;
    CNN_KLAUNCH(s, "clip_finish", (clip_finish<<<1, kBlock, 0, s>>>(partial, (int)partials, max_norm, grad_scale, grad_scale != 1.0f, stats_dev)),
                "partials=%u", partials);
    return launch_stream(
        s, "clip_scale_vec", "clip_scale_scalar", kClip, aligned, n, -1,
        [&](unsigned grid, size_t) { clip_scale<true><<<grid, kBlock, 0, s>>>(grads, n, stats_dev); },
        [&](unsigned grid, size_t) { clip_scale<false><<<grid, kBlock, 0, s>>>(grads, n, stats_dev); });
}

int cnn_softmax_xent(const float* logits, const int32_t* labels, float* probs, float* delta, float* loss_sum, int B,
                     int classes, void* stream) {
    CNN_REQUIRE(logits && labels && delta, "cnn_softmax_xent: null pointer");
    CNN_REQUIRE(B > 0 && classes > 0, "cnn_softmax_xent: B=%d classes=%d", B, classes);
    hipStream_t s = as_stream(stream);
    CNN_KLAUNCH(s, "softmax_xent_kernel",
                (softmax_xent_kernel<false><<<1, kBlock, 0, s>>>(logits, labels, probs, delta, loss_sum, B, classes)), "B=%d classes=%d",
                B, classes);
    return CNN_AMD_OK;
}

int cnn_softmax_xent_soft(const float* logits, const float* targets, float* probs, float* delta, float* loss_sum, int B, int classes,
                          void* stream) {
    CNN_REQUIRE(logits && targets && delta, "cnn_softmax_xent_soft: null pointer");
    CNN_REQUIRE(B > 0 && classes > 0, "cnn_softmax_xent_soft: B=%d classes=%d", B, classes);
    hipStream_t s = as_stream(stream);
    CNN_KLAUNCH(s, "softmax_xent_soft_kernel",
                (softmax_xent_kernel<true><<<1, kBlock, 0, s>>>(logits, targets, probs, delta, loss_sum, B, classes)), "B=%d classes=%d", B,
                classes);
    return CNN_AMD_OK;
}

// the partner rule of cnn_soft_targets / cnn_batch_mix, checked on the host: the rule is known, a ROLL shift lies in [1, B)
static int check_pair_rule(const char* entry, int B, int pair_rule, int pair_shift) {
    CNN_REQUIRE(pair_rule == CNN_PAIR_NONE || pair_rule == CNN_PAIR_FLIP || pair_rule == CNN_PAIR_ROLL, "%s: unknown pair_rule=%d", entry, pair_rule);
    CNN_REQUIRE(pair_rule != CNN_PAIR_ROLL || (pair_shift >= 1 && pair_shift < B), "%s: CNN_PAIR_ROLL shift=%d outside [1, B=%d)", entry, pair_shift, B);
    return CNN_AMD_OK;
}

int cnn_soft_targets(const int32_t* labels, float* targets, int B, int classes, float smoothing, float lam, int pair_rule, int pair_shift,
                     void* stream) {
    CNN_REQUIRE(labels && targets, "cnn_soft_targets: null pointer");
    CNN_REQUIRE(B > 0 && classes > 0, "cnn_soft_targets: B=%d classes=%d", B, classes);
    CNN_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "cnn_soft_targets: smoothing=%g outside [0, 1)", (double)smoothing);
    CNN_REQUIRE(lam >= 0.f && lam <= 1.f, "cnn_soft_targets: lam=%g outside [0, 1]", (double)lam);
    if (int rc = check_pair_rule("cnn_soft_targets", B, pair_rule, pair_shift)) return rc;
    SoftTargetArgs a;
    a.B = B;
    a.classes = classes;
    a.smooth = smoothing != 0.f;
    const volatile float u = smoothing / (float)classes;  // (volatile: every operation rounded to fp32 on its own)
    const volatile float keep = 1.f - smoothing;
    a.u = u;
    a.hot = keep + u;
    a.lam = lam;
    a.oml = 1.f - lam;
    a.rule = lam == 1.f ? CNN_PAIR_NONE : pair_rule;
    a.shift = pair_shift;
    hipStream_t s = as_stream(stream);
    const size_t n = (size_t)B * classes;
    CNN_KLAUNCH(s, "soft_targets_kernel", (soft_targets_kernel<<<stream_grid(n, kBlock), kBlock, 0, s>>>(labels, targets, a)), "B=%d classes=%d rule=%d", B,
                classes, a.rule);
    return CNN_AMD_OK;
}

float cnn_cutmix_lambda(int H, int W, int y0, int y1, int x0, int x1) {
    return (float)(1.0 - (double)((long long)(y1 - y0) * (x1 - x0)) / ((double)H * W));
}

int cnn_batch_mix(const cnn_mix_desc* d, const float* src, float* dst, int B, int C, int H, int W, void* stream) {
    CNN_REQUIRE(d && src && dst, "cnn_batch_mix: null pointer");
    CNN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "cnn_batch_mix: B=%d C=%d H=%d W=%d", B, C, H, W);
    CNN_REQUIRE((long long)C * H * W < (1ll << 31), "cnn_batch_mix: a sample of C=%d H=%d W=%d exceeds 2^31 - 1 elements", C, H, W);
    CNN_REQUIRE(d->mode == CNN_MIX_MIXUP || d->mode == CNN_MIX_CUTMIX, "cnn_batch_mix: unknown mode=%d", d->mode);
    if (int rc = check_pair_rule("cnn_batch_mix", B, d->pair_rule, d->pair_shift)) return rc;
    if (d->mode == CNN_MIX_MIXUP)
        CNN_REQUIRE(d->lam >= 0.f && d->lam <= 1.f, "cnn_batch_mix: lam=%g outside [0, 1]", (double)d->lam);
    else
        CNN_REQUIRE(0 <= d->y0 && d->y0 <= d->y1 && d->y1 <= H && 0 <= d->x0 && d->x0 <= d->x1 && d->x1 <= W,
                    "cnn_batch_mix: box y=[%d, %d) x=[%d, %d) outside the %d x %d plane or reversed", d->y0, d->y1, d->x0, d->x1, H, W);
    const size_t ns = (size_t)C * H * W, n = ns * (size_t)B;
    CNN_REQUIRE(!floats_overlap(dst, src, n), "cnn_batch_mix: dst and src are the same buffer or overlap");
    hipStream_t s = as_stream(stream);
    const bool aligned = aligned16(src) && aligned16(dst);
    const bool empty_box = d->mode == CNN_MIX_CUTMIX && (d->y0 == d->y1 || d->x0 == d->x1);
    if (d->pair_rule == CNN_PAIR_NONE || empty_box || (d->mode == CNN_MIX_MIXUP && d->lam == 1.f))  // nothing is mixed: the copy of the bits
        return launch_stream(s, "bmix_copy_vec", gacc_vec<true>, "bmix_copy_scalar", gacc_scalar<true>, kTailRides, aligned, n, -1, GaccOp<true>{dst, src});
    // a sample per grid row (the partner is workgroup-uniform), the walker inside the sample; the float4 form where every sample starts
    // 16-byte aligned
    BmixArgs a;
    a.ns = ns;
    a.B = B;
    a.rule = d->pair_rule;
    a.shift = d->pair_shift;
    const auto grid = [&](size_t work_items) {
        const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
        const unsigned want = stream_grid(work_items * gy, kBlock), gx = (want + gy - 1) / gy;
        const unsigned need = (unsigned)((work_items + kBlock - 1) / kBlock);
        return dim3(gx < need ? gx : need, gy);
    };
    const bool vec = aligned && ns % 4 == 0;
    if (d->mode == CNN_MIX_MIXUP) {
        const float lam = d->lam, oml = 1.f - d->lam;
        return launch_stream(
            s, "bmix_mixup_vec", "bmix_mixup_scalar", kTailRides, vec, ns, -1,
            [&](unsigned, size_t) { bmix_mixup<true><<<grid(ns / 4), kBlock, 0, s>>>(src, dst, a, lam, oml); },
            [&](unsigned, size_t) { bmix_mixup<false><<<grid(ns), kBlock, 0, s>>>(src, dst, a, lam, oml); });
    }
    const CutBox box{(uint32_t)H, (uint32_t)W, (uint32_t)d->y0, (uint32_t)d->y1, (uint32_t)d->x0, (uint32_t)d->x1};
    return launch_stream(
        s, "bmix_cutmix_vec", "bmix_cutmix_scalar", kTailRides, vec, ns, -1,
        [&](unsigned, size_t) { bmix_cutmix<true><<<grid(ns / 4), kBlock, 0, s>>>(src, dst, a, box); },
        [&](unsigned, size_t) { bmix_cutmix<false><<<grid(ns), kBlock, 0, s>>>(src, dst, a, box); });
}

int cnn_dropout_forward(const float* x, float* y, int B, int C, int H, int W, int dropped_channels, int training, float keep,
                        void* stream) {
    CNN_REQUIRE(x && y && B > 0 && C > 0 && H > 0 && W > 0 && dropped_channels >= 0 && dropped_channels <= C, "cnn_dropout_forward: bad arguments");
    const size_t n = (size_t)B * C * H * W;
    hipStream_t s = as_stream(stream);
    CNN_KLAUNCH(s, "dropout_fwd", (dropout_fwd<<<stream_grid(n, kBlock), kBlock, 0, s>>>(DropoutFwdOp{x, y, C, H * W, dropped_channels, training, keep}, n)),
                "n=%zu", n);
    return CNN_AMD_OK;
}

int cnn_dropout_backward(float* dy_inout, int B, int C, int H, int W, int dropped_channels, void* stream) {
    CNN_REQUIRE(dy_inout && B > 0 && C > 0 && H > 0 && W > 0 && dropped_channels >= 0 && dropped_channels <= C, "cnn_dropout_backward: bad arguments");
    const size_t n = (size_t)B * C * H * W;
    hipStream_t s = as_stream(stream);
    CNN_KLAUNCH(s, "dropout_bwd", (dropout_bwd<<<stream_grid(n, kBlock), kBlock, 0, s>>>(DropoutBwdOp{dy_inout, C, H * W, dropped_channels}, n)), "n=%zu", n);
    return CNN_AMD_OK;
}


int cnn_grad_cam(const float* feature, int B, int C, int H, int W, float* cam, unsigned char* image, void* stream) {
    CNN_REQUIRE(feature && cam, "cnn_grad_cam: null pointer");
    CNN_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "cnn_grad_cam: B=%d C=%d H=%d W=%d", B, C, H, W);
    CNN_REQUIRE((size_t)C * sizeof(float) <= 64 * 1024, "cnn_grad_cam: C=%d channels exceed the 64 KB weight table", C);
    hipStream_t s = as_stream(stream);
    const int area = H * W;
    CNN_KLAUNCH(s, "grad_cam_maps", (grad_cam_maps<<<B, kBlock, (size_t)C * sizeof(float), s>>>(feature, cam, C, area)), "B%d C%d %dx%d", B, C, H, W);
    CNN_KLAUNCH(s, "grad_cam_normalise", (grad_cam_normalise<<<1, kBlock, 0, s>>>(cam, image, (size_t)B * area, area)), "n=%zu", (size_t)B * area);
    return CNN_AMD_OK;
}

}  // extern "C"
