// common.h -- shared host-side helpers for the libcnn_amd.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cfloat>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "cnn_amd.h"
#include "stager_layout.h"

namespace cnn_amd {

// last-error text (per thread), surfaced through cnn_amd_last_error()
char* error_buffer();
int fail(int code, const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Memo of a planning result per (desc, option-table generation), per host thread: the size queries walk every tile candidate of the
// implicit GEMM (34 plans) and are called by the prepared entry points and the host layers on EVERY launch -- 800+ plans per train step
// of the reference net, most of the 0.36 ms the host needed to enqueue a 0.39 ms step.
unsigned options_generation();
int num_cus();
struct DescMemo {
    struct Entry {
        cnn_conv2d_desc d;
        unsigned gen;
        int cus;  // (the planners size their grids by the CURRENT device's CU count: a thread that changes devices must not hit)
        bool used;
        size_t value;
    };
    Entry e[16] = {};
    int next = 0;
    bool find(const cnn_conv2d_desc* d, size_t* out) const {
        const unsigned gen = options_generation();
        const int cus = num_cus();
        for (const Entry& x : e)
            if (x.used && x.gen == gen && x.cus == cus && x.d.B == d->B && x.d.Ci == d->Ci && x.d.H == d->H && x.d.W == d->W && x.d.Co == d->Co && x.d.k == d->k &&
                x.d.s == d->s && x.d.pad == d->pad && x.d.flags == d->flags) {
                *out = x.value;
                return true;
            }
        return false;
    }
    void put(const cnn_conv2d_desc* d, size_t v) {
        e[next] = Entry{*d, options_generation(), num_cus(), true, v};
        next = (next + 1) % 16;
    }
};

// packed pool mask (include/cnn_amd.h, CNN_CONV2D_POOL_MASK_PACKED): bytes per pooled row (rows start 4-byte aligned: the window
// kernel moves four windows' bytes per 4-byte LDS-DMA)
__host__ __device__ inline int pool_mask_pitch(int PWo) { return (PWo + 3) & ~3; }

// ---- measurement switches -------------------------------------------------------------------------------
// The A/B switches of the kernels' planners live in ONE process-wide table (abi.hip): filled once from the CNN_AMD_* variables of the
// environment when the library is first used, changed afterwards only through cnn_amd_set_option() (include/cnn_amd.h).  A launch
// path never calls getenv: a site holds a static Option whose cached value is re-read from the table only when the table's
// generation counter has moved (one relaxed atomic load per query otherwise).  Names are the variable names without "CNN_AMD_".
unsigned options_generation();
bool option_lookup(const char* name, long long* ival, double* dval);  // false: not set
class Option {
public:
    explicit Option(const char* n) : name_(n) {}
    bool is_set() { refresh(); return set_.load(std::memory_order_relaxed); }
    int as_int(int dflt) { refresh(); return set_.load(std::memory_order_relaxed) ? (int)ival_.load(std::memory_order_relaxed) : dflt; }
    double as_double(double dflt) { refresh(); return set_.load(std::memory_order_relaxed) ? dval_.load(std::memory_order_relaxed) : dflt; }
private:
    void refresh() {
        const unsigned g = options_generation();
        if (gen_.load(std::memory_order_acquire) == g) return;
        long long iv = 0;
        double dv = 0;
        const bool s = option_lookup(name_, &iv, &dv);
        ival_.store(iv, std::memory_order_relaxed);
        dval_.store(dv, std::memory_order_relaxed);
        set_.store(s, std::memory_order_relaxed);
        gen_.store(g, std::memory_order_release);
    }
    const char* name_;
    std::atomic<unsigned> gen_{0};  // (the table's generation starts at 1)
    std::atomic<bool> set_{false};
    std::atomic<long long> ival_{0};
    std::atomic<double> dval_{0};
};
// one static Option per call site
#define CNN_OPT(name) ([]() -> ::cnn_amd::Option& { static ::cnn_amd::Option o__(name); return o__; }())
#define CNN_OPT_SET(name) (CNN_OPT(name).is_set())
#define CNN_OPT_INT(name, dflt) (CNN_OPT(name).as_int(dflt))
// "is it set, and to which integer" in one value: `const OptVal e = CNN_OPT_VAL("X"); if (e && atoi(e) == 0) ...`
struct OptVal {
    bool set;
    int v;
    explicit operator bool() const { return set; }
};
inline int atoi(const OptVal& o) { return o.v; }
inline OptVal opt_val(Option& o) { return OptVal{o.is_set(), o.as_int(0)}; }
#define CNN_OPT_VAL(name) (::cnn_amd::opt_val(CNN_OPT(name)))

// MEASUREMENT-ONLY switches: ablations that leave out a kernel's stores / DMAs / MFMAs, per-phase cycle printers, an
// LDS request override, a data-parallel step without its exchange -- anything that changes RESULTS or exists for a timing experiment.
// They exist only in the measurement build (make -C cnn_amd/csrc measure -> libcnn_amd_measure.so, -DCNN_AMD_MEASURE, used by tools/);
// in the product library every such query is the compile-time constant `dflt`, cnn_amd_set_option() rejects the names and the
// CNN_AMD_* environment is not consulted for them (abi.hip: kMeasureOnly; tests/test_abi_exports.py).
#ifdef CNN_AMD_MEASURE
#define CNN_MEASURE_INT(name, dflt) CNN_OPT_INT(name, dflt)
#else
#define CNN_MEASURE_INT(name, dflt) (dflt)
#endif
bool measure_only_option(const char* name);  // (abi.hip) is `name` one of them

// compute units of the current device (hipDeviceProp_t::multiProcessorCount, cached per device; 256 on MI355X), or the smaller
// count the switch CUS asks for (abi.hip)
int num_cus();

#define CNN_HIP_CHECK(expr)                                                                         \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return ::cnn_amd::fail(CNN_AMD_E_HIP + (int)e__, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// every kernel launch is followed by this: catches bad launch configs without synchronising
#define CNN_LAUNCH_CHECK() CNN_HIP_CHECK(hipGetLastError())

// Optional per-kernel timing with HIP events recorded on the launch stream (cnn_amd_kernel_timing_* in the ABI).
// mode 0 = off (one predictable branch per launch), 1 = every kernel, 2 = only records whose key contains `filter`.
bool ktimer_active();
void ktimer_begin(hipStream_t s, const char* kernel, const char* fmt, ...);
void ktimer_end(hipStream_t s);

// ---- "published" kernels: a cross-stream dependency without a marker packet on the producing stream -------------------------
// hipEventRecord between two kernels of one stream costs that stream ~4.5 us (measured, tools/micro/event_gap.hip: the marker
// packet has to retire before the next dispatch); an event attached to the producing kernel's OWN dispatch packet
// (hipExtLaunchKernelGGL's stopEvent) costs ~1.7 us and releases the waiting stream ~4 us sooner.  cnn_amd_publish_next_kernel(stream)
// arms the calling thread: the next kernel the library launches on `stream` carries the event -- through launch_pub() at the launch
// sites that sit in front of a fork in the train step, through a plain hipEventRecord behind any other launch (same meaning,
// old cost).  Consumers: cnn_amd_wait_published(), and the fork of cnn_conv2d_backward*(defer_join = 2).
struct PublishState {
    hipEvent_t ev[2] = {nullptr, nullptr};
    int cur = 0, device = -1;
    bool armed = false;   // the next launch on `stream` publishes
    bool valid = false;   // ev[cur] marks the completion of the last published kernel ...
    bool stale = false;   // ... but the library has launched something else on that stream since
    hipStream_t stream = nullptr;
};
PublishState& publish_state();                   // per host thread (abi.hip)
hipEvent_t publish_take(hipStream_t s);          // armed for s: the event to attach (state -> published), else nullptr
int publish_after_launch(hipStream_t s);         // bookkeeping behind EVERY launch (fallback record / staleness)
void publish_mark_stale(hipStream_t s);         // something that is NOT a library kernel was queued on s (copies, waits, collectives)
inline bool publish_busy() {
    const PublishState& p = publish_state();
    return p.armed || (p.valid && !p.stale);
}

// kernel launch that can carry the published event (use inside CNN_KLAUNCH instead of kernel<<<...>>>(...))
template <typename... KArgs, typename... Args>
inline void launch_pub(void (*kern)(KArgs...), dim3 grid, dim3 block, unsigned shmem, hipStream_t s, Args&&... args) {
    hipEvent_t ev = publish_take(s);
    if (ev) hipExtLaunchKernelGGL(kern, grid, block, shmem, s, nullptr, ev, 0, static_cast<KArgs>(args)...);
    else hipLaunchKernelGGL(kern, grid, block, shmem, s, static_cast<KArgs>(args)...);
}

// launch `expr` (a kernel<<<...>>>(...) expression), timed when profiling is on; `...` = printf-style geometry tag
#define CNN_KLAUNCH(stream, kernel_name, expr, ...)                                         \
    do {                                                                                    \
        const bool t__ = ::cnn_amd::ktimer_active();                                        \
        if (t__) ::cnn_amd::ktimer_begin(stream, kernel_name, __VA_ARGS__);                 \
        expr;                                                                               \
        if (t__) ::cnn_amd::ktimer_end(stream);                                             \
        CNN_LAUNCH_CHECK();                                                                 \
        if (::cnn_amd::publish_busy())                                                      \
            if (int prc__ = ::cnn_amd::publish_after_launch(stream)) return prc__;          \
    } while (0)

#define CNN_REQUIRE(cond, ...)                                             \
    do {                                                                   \
        if (!(cond)) return ::cnn_amd::fail(CNN_AMD_E_BADARG, __VA_ARGS__); \
    } while (0)

// conv_dgrad_rd.hip's m16 kernel keeps the filters of a 16-input-channel slice as MFMA A operands: register j = c4*9 + tap
// (0 .. 2.25*Co - 1) of lane l = (ci = l & 15, k = l >> 4) holds w[4*c4 + k][16*slice + ci][tap] ([Co][Ci][3][3] layout).
// The prepared copy is img[(slice*NA + j)*64 + l], NA = 2.25*Co (one coalesced load per j).
__host__ __device__ inline int m16_filter_index(int j, int lane, int Ci, int slice) {
    return ((4 * (j / 9) + (lane >> 4)) * Ci + 16 * slice + (lane & 15)) * 9 + j % 9;
}

// "has this per-function attribute been set on the CURRENT device yet" (hipFuncSetAttribute is per device): one atomic flag per
// device and call site.  (racing threads may both set it: setting the attribute twice is
// harmless, never setting it on a second device -- or launching before it is set -- is not): needed() until mark().
struct DeviceOnce {
    std::atomic<unsigned char> done[64];
    static int device() {
        int dev = 0;
        return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) ? dev : -1;
    }
    bool needed() const {
        const int dev = device();
        return dev < 0 || done[dev].load(std::memory_order_acquire) == 0;
    }
    void mark() {
        const int dev = device();
        if (dev >= 0) done[dev].store(1, std::memory_order_release);
    }
};
// let `kernels` request up to `bytes` of dynamic LDS on the current device, once per device and `once` flag (one flag per call site
// and template instance).  A failed call leaves the flag unmarked: `if (int rc = allow_dynamic_lds(...)) return rc;`
template <class... K>
inline int allow_dynamic_lds(DeviceOnce& once, int bytes, K... kernels) {
    if (!once.needed()) return CNN_AMD_OK;
    for (const void* kern : {(const void*)kernels...}) CNN_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    once.mark();
    return CNN_AMD_OK;
}

// `total` work units over `want` workgroups (clamped to 1 .. total): units per workgroup, rounded up, and the workgroups that leaves
inline void split_units(long long total, long long want, int* per_block, int* blocks) {
    if (want < 1) want = 1;
    if (want > total) want = total;
    *per_block = (int)((total + want - 1) / want);
    *blocks = (int)((total + *per_block - 1) / *per_block);
}

// SGD on one element (alexnet.cpp:62-65, conv2d.cpp / linear.cpp update_gradients):
// p - lr*(g*scale) with every product/sum rounded separately: the reference is built without FMA
// (x86-64 -O2, CMakeLists.txt:5), so w -= lr*g is mul-then-sub; the fp-contract pragma stops hipcc fusing it
// (HIP's __fmul_rn/__fsub_rn are plain operators and do get contracted).
__device__ __forceinline__ float sgd_one(float p, float g, float lr, float scale, bool scaled) {
#pragma clang fp contract(off)
    const float gs = scaled ? g * scale : g;
    const float step = lr * gs;
    return p - step;
}

// SGD with momentum / weight decay / Nesterov on one element (cnn_sgd_momentum_update, include/cnn_amd.h has the formula): the
// arithmetic of torch.optim.SGD (dampening 0) in sgd_one's manner -- fp32, every product and sum rounded separately.  `decay` = this
// element is inside a decayed range AND weight_decay != 0.  kMomentum = false: v is neither read nor written, and with decay false
// the result is sgd_one's bit for bit.
template <bool kMomentum>
__device__ __forceinline__ float sgdm_one(float p, float g, float& v, float lr, float momentum, float wd, float scale, bool scaled,
                                          bool decay, bool nesterov) {
#pragma clang fp contract(off)
    const float gs = scaled ? g * scale : g;
    float d = gs;
    if (decay) {
        const float wp = wd * p;
        d = gs + wp;
    }
    float u = d;
    if (kMomentum) {
        const float mv = momentum * v;
        const float vn = mv + d;
        v = vn;
        if (nesterov) {
            const float mvn = momentum * vn;
            u = d + mvn;
        } else {
            u = vn;
        }
    }
    const float step = lr * u;
    return p - step;
}

// Adam / AdamW on one element (cnn_adam_update, include/cnn_amd.h has the formula): the arithmetic of torch.optim.Adam / AdamW
// (amsgrad off) in sgdm_one's manner -- fp32, every product, sum, quotient and root rounded separately; the quotient and the root
// are the correctly rounded ones (no fast-math flag in the build), denormals are kept.  The scalars that do not depend on the
// element are computed once on the host (cnn_adam_update):
//     om   = 1.f - lr * weight_decay                                  (two fp32 operations)
//     omb1 = 1.f - beta1,  omb2 = 1.f - beta2                         (fp32)
//     bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step))
//     ss   = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)))
// Per element, `decay` = inside a decayed range AND weight_decay != 0:
//     gs  = scaled ? g * scale : g
//     d   = (decay && !decoupled) ? gs + wd * p : gs
//     p0  = (decay &&  decoupled) ? p * om : p
//     m'  = beta1 * m + omb1 * d
//     v'  = beta2 * v + omb2 * (d * d)
//     den = sqrt(v') / bc2s + eps
//     q   = m' / den
//     p'  = p0 - ss * q
struct AdamScalars {
    float beta1, beta2, omb1, omb2, eps, wd, om, bc2s, ss, scale;
    bool scaled, decoupled;
};
__device__ __forceinline__ float adam_one(float p, float g, float& m, float& v, const AdamScalars& a, bool decay) {
#pragma clang fp contract(off)
    const float gs = a.scaled ? g * a.scale : g;
    float d = gs;
    float p0 = p;
    if (decay) {
        if (a.decoupled) {
            p0 = p * a.om;
        } else {
            const float wp = a.wd * p;
            d = gs + wp;
        }
    }
    const float b1m = a.beta1 * m;
    const float o1d = a.omb1 * d;
    const float mn = b1m + o1d;
    const float b2v = a.beta2 * v;
    const float dd = d * d;
    const float o2d = a.omb2 * dd;
    const float vn = b2v + o2d;
    m = mn;
    v = vn;
    const float root = sqrtf(vn);
    const float rb = root / a.bc2s;
    const float den = rb + a.eps;
    const float q = mn / den;
    const float step = a.ss * q;
    return p0 - step;
}

// LAMB on one element (cnn_lamb_update, include/cnn_amd.h has the formula): Adam's moments with a per-tensor trust ratio, in
// adam_one's arithmetic -- fp32, every product, sum, quotient and root rounded separately, correctly rounded quotients and roots,
// denormals kept.  The step is two element passes with the segment norms in between.  Host scalars (cnn_lamb_update):
//     omb1 = 1.f - beta1,  omb2 = 1.f - beta2                         (fp32)
//     bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step))
//     bc1  = (float)(1.0 - pow((double)beta1, (double)step))
// First pass, `decay` = the element's segment has CNN_SEG_DECAY AND weight_decay != 0; the result r goes to the `update` scratch:
//     gs  = scaled ? g * scale : g
//     m'  = beta1 * m + omb1 * gs
//     v'  = beta2 * v + omb2 * (gs * gs)
//     den = sqrt(v') / bc2s + eps
//     mh  = m' / bc1
//     q   = mh / den
//     r   = decay ? q + wd * p : q
struct LambScalars {
    float beta1, beta2, omb1, omb2, eps, wd, bc2s, bc1, scale;
    bool scaled;
};
__device__ __forceinline__ float lamb_moments_one(float p, float g, float& m, float& v, const LambScalars& a, bool decay) {
#pragma clang fp contract(off)
    const float gs = a.scaled ? g * a.scale : g;
    const float b1m = a.beta1 * m;
    const float o1g = a.omb1 * gs;
    const float mn = b1m + o1g;
    const float b2v = a.beta2 * v;
    const float gg = gs * gs;
    const float o2g = a.omb2 * gg;
    const float vn = b2v + o2g;
    m = mn;
    v = vn;
    const float root = sqrtf(vn);
    const float rb = root / a.bc2s;
    const float den = rb + a.eps;
    const float mh = mn / a.bc1;
    const float q = mh / den;
    float r = q;
    if (decay) {
        const float wp = a.wd * p;
        r = q + wp;
    }
    return r;
}
// Second pass, ratio = the trust ratio of the element's segment (exactly 1 where it does not apply):
//     t  = ratio * r
//     p' = p - lr * t
__device__ __forceinline__ float lamb_apply_one(float p, float r, float ratio, float lr) {
#pragma clang fp contract(off)
    const float t = ratio * r;
    const float step = lr * t;
    return p - step;
}

// LARS on one element (cnn_lars_update, include/cnn_amd.h has the formula): sgdm_one with the trust ratio of the element's segment
// on the decayed gradient.  `decay` = the segment has CNN_SEG_DECAY AND weight_decay != 0.
//     gs = scaled ? g * scale : g
//     d  = decay ? gs + wd * p : gs
//     dl = ratio * d
//     momentum == 0 :  u = dl
//     otherwise     :  v' = momentum * v + dl ;  u = nesterov ? dl + momentum * v' : v'
//     p' = p - lr * u
// x * 1.0f is exact: with ratio = 1 the result is sgdm_one's bit for bit.
template <bool kMomentum>
__device__ __forceinline__ float lars_one(float p, float g, float& v, float ratio, float lr, float momentum, float wd, float scale, bool scaled,
                                          bool decay, bool nesterov) {
#pragma clang fp contract(off)
    const float gs = scaled ? g * scale : g;
    float d = gs;
    if (decay) {
        const float wp = wd * p;
        d = gs + wp;
    }
    const float dl = ratio * d;
    float u = dl;
    if (kMomentum) {
        const float mv = momentum * v;
        const float vn = mv + dl;
        v = vn;
        if (nesterov) {
            const float mvn = momentum * vn;
            u = dl + mvn;
        } else {
            u = vn;
        }
    }
    const float step = lr * u;
    return p - step;
}

// the reference's exp of a softmax row (func.cpp:6-12): shared by softmax_xent_kernel (elementwise.hip) and eval_accumulate
// (metrics.hip), whose loss terms must have the same bits
__device__ __forceinline__ float clamped_exp(float v) {
    if (v >= 88.f) return FLT_MAX;
    if (v <= -50.f) return 0.f;
    return expf(v);
}

constexpr int kWave = 64;         // CDNA wavefront
constexpr int kNumXCD = 8;

// Workgroups are dealt round-robin to the 8 XCDs (id % 8), each with its own L2: neighbouring tiles of an image -- which share
// halo rows -- would sit on eight different L2s and fetch those rows eight times.  This gives XCD x the x-th CONTIGUOUS eighth of
// the logical ids instead (same bijection as the implicit GEMM's tile map).  nb = gridDim.x.
__device__ __forceinline__ unsigned xcd_swizzle(unsigned bid, unsigned nb) {
#ifdef CNN_NO_XCD_SWIZZLE  // (A/B builds only)
    return bid;
#endif
    const unsigned q = nb / kNumXCD, r = nb % kNumXCD, xcd = bid % kNumXCD, k = bid / kNumXCD;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

inline unsigned ceil_div(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// the float4 kernels need 16-byte aligned pointers; the entries fall back to their scalar forms (or refuse) otherwise
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// grid for HBM-bound streaming kernels: enough workgroups to fill 256 CUs x 8, grid-stride the rest
inline unsigned stream_grid(size_t work_items, int block) {
    size_t need = (work_items + block - 1) / block;
    size_t cap = (size_t)num_cus() * 8;
    return (unsigned)(need < 1 ? 1 : (need > cap ? cap : need));
}

// One level of a dataset with half-size levels (cnn_dataset_create_u8_levels): where its [N][H][W][3] region begins in the store, its
// size and the bytes of one sample (H * W * 3).  The dataset (staging.hip) keeps a host and a device copy of the table.
struct DatasetLevel {
    long long base;
    int H, W;
    int sample_bytes;
    int reserved;
};

}  // namespace cnn_amd

// The two argument blocks of augment.hip's kernel template beside the pointers.  Unnamed namespace on purpose: a kernel's symbol spells
// the types of its parameters, and with internal linkage here the symbols are the same whichever file fills the blocks.
namespace {
struct PhotoNorm {  // the photo stager's normalisation: out = u * s[c] + t[c], u clamped to [0, 1] first if `clamp`
    float s[3], t[3];
    int clamp;
};
struct ResidentArgs {
    const int* indices;  // [B], device; null: the source is the batch's own images
    const int* labels;   // [N], the dataset's
    int* labels_out;     // [B]
    long long N;
    // levels only (`levels` non-null): the sample's level, and the dataset's table of levels (device memory: a by-value array indexed by
    // a runtime level would live in scratch)
    const int* levels;                   // [B], device
    const cnn_amd::DatasetLevel* table;  // [L]
    int L;
};
}  // namespace

namespace cnn_amd {

// augment.hip: one launch of the augmenting gather per batch, for cnn_augment_u8 and for the submit() of the augmenting stagers
// (staging.hip).  src: [B][Hs][Ws][3] device bytes, or a dataset's store when res.indices is set (Hs, Ws: level 0's; with res.levels set
// `mats` holds the LEVEL maps of cnn_augment_level).  photo ([B][20], device) is null for the plain gather.  augment_u8_run checks
// pointers, sizes and fill, and names `who` in the message.
struct AugmentJob {
    const unsigned char* src;
    int B, Hs, Ws;
    const float* mats;  // [B][6], device
    float fill;
    float* dst;  // [B][3][H][W]
    int H, W;
    const float* photo;
    PhotoNorm norm;
    ResidentArgs res;
};
int augment_u8_run(const char* who, const AugmentJob& job, hipStream_t stream);
// lut[v] = v * 1.f / 255 evaluated on the host, on the current device: one copy per device, made at first use, kept for the process
int device_lut(const float** out);
// level l of samples [first, first + count) from level l - 1 (dataset_halve_u8): src [N][Hp][Wp][3], dst [N][(Hp+1)/2][(Wp+1)/2][3]
int dataset_halve_u8(const unsigned char* src, unsigned char* dst, long long first, long long count, int Hp, int Wp, hipStream_t stream);

}  // namespace cnn_amd
