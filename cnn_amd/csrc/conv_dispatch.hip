// conv_dispatch.hip -- which kernel family runs a Conv2D forward or data gradient (host code only).
//
// Each pass has ONE ordered table of routes, kFwdRoutes / kDgradRoutes below.  A route says whether its family covers a desc under
// the current option table, what it needs from the buffer the caller hands over, what its prepared filter image is and how to run
// it.  resolve() picks the first route that applies and fits the buffer, and everything goes through it: the run entry points,
// cnn_conv2d_prepare_filters (against the prepared buffer it was handed, so the image it writes is by construction the one the
// *_prepared call will read), the size queries (the largest image over the routes) and the "is there a prepared path / a
// ReLU-only output" questions.  A new family is one row per pass.
#include "conv_families.h"

using namespace cnn_amd;

namespace {

enum BufferNeed { NEED_NOTHING, NEED_FLOATS, NEED_FLOATS_ALIGNED16 };  // of Route::floats(d) floats; unmet: the next route
enum ImageKind { IMAGE_NONE, IMAGE_COPY_OF_W, IMAGE_PACKED };          // none: the layer has no *_prepared path

// one call of a pass.  forward: in = x, out = y (nullable where the route allows), out2 = relu(y) (nullable);
// data gradient: in = dy, out = dx, out2 = output of the ReLU layer below (nullable: its backward pass is fused in)
struct ConvCall {
    const char* who;
    const cnn_conv2d_desc* d;
    const float* in;
    const float* w;  // unused when prepared: `ws` then holds the route's image
    const float* bias;
    float* out;
    float* out2;
    void* ws;
    size_t ws_bytes;
    hipStream_t s;
    bool prepared;
    const float* image() const { return (const float*)ws; }
    const float* w_or_copy() const { return prepared ? (const float*)ws : w; }  // routes whose image is a verbatim copy of w
};

typedef int (*PrepareBatchFn)(int n, const ConvPrepJob* jobs, hipStream_t s);

struct Route {
    bool (*applies)(const cnn_conv2d_desc* d);
    BufferNeed need;
    ImageKind (*image)(const cnn_conv2d_desc* d);
    size_t (*floats)(const cnn_conv2d_desc* d);  // of the prepared image (= what `need` asks of the buffer)
    PrepareBatchFn prepare;                      // IMAGE_PACKED: writes the images of the jobs that resolved here, one launch
    int (*run)(const ConvCall& c);
    bool needs_y;  // forward: cannot write the ReLU output alone
};

ImageKind packed(const cnn_conv2d_desc*) { return IMAGE_PACKED; }
ImageKind copy_of_w(const cnn_conv2d_desc*) { return IMAGE_COPY_OF_W; }
size_t filter_floats(const cnn_conv2d_desc* d) { return (size_t)d->Co * d->Ci * d->k * d->k; }
size_t direct_floats(const cnn_conv2d_desc*) { return 1024; }  // packed filter copies of the first-layer kernels (conv_direct.hip)
bool always(const cnn_conv2d_desc*) { return true; }
ImageKind no_image(const cnn_conv2d_desc*) { return IMAGE_NONE; }
size_t no_floats(const cnn_conv2d_desc*) { return 0; }

int thin_pack_jobs(int n, const ConvPrepJob* jobs, hipStream_t s) {
    for (int i = 0; i < n; ++i)
        if (int rc = thin_dgrad_pack(jobs[i].d, jobs[i].w, jobs[i].image, s)) return rc;
    return CNN_AMD_OK;
}

int run_rows(const ConvCall& c, int mode) {
    if (!c.prepared)
        if (int rc = rows_prepare(c.d, mode, c.w, (float*)c.ws, c.s)) return rc;
    return rows_run(c.d, mode, c.in, c.image(), mode == MODE_FWD ? c.bias : nullptr, c.out, mode == MODE_FWD ? c.out2 : nullptr,
                    mode == MODE_FWD ? nullptr : c.out2, c.s);
}

// ---- forward: depthwise (iff the desc carries the flag: no later row ever sees such a desc, see facts_of) -> direct -> 1x1 -> rows ->
// fwd_rd -> stem -> implicit GEMM ----
const Route kFwdRoutes[] = {
    /* depthwise */ {is_depthwise, NEED_NOTHING, no_image, no_floats, nullptr,
     [](const ConvCall& c) { return dw_run(c.d, MODE_FWD, c.in, c.w, c.bias, c.out, c.out2, c.s); }, false},
    /* direct */ {direct_conv_supported, NEED_NOTHING,  // (picks its packed or its plain kernel by the buffer itself)
     [](const cnn_conv2d_desc* d) { return direct_fwd_pk_ok(d) ? IMAGE_PACKED : IMAGE_NONE; }, direct_floats, direct_prepare_batch,
     [](const ConvCall& c) { return direct_conv_forward(c.d, c.in, c.w, c.bias, c.out, c.out2, c.ws, c.ws_bytes, c.s, c.prepared); }, true},
    /* 1x1 */ {c11_supported, NEED_NOTHING, copy_of_w, filter_floats, nullptr,
     [](const ConvCall& c) { return c11_forward(c.d, c.in, c.w_or_copy(), c.bias, c.out, c.out2, c.s); }, false},
    /* rows */ {[](const cnn_conv2d_desc* d) { return rows_workspace_floats(d, MODE_FWD) > 0; }, NEED_FLOATS_ALIGNED16, packed,
     [](const cnn_conv2d_desc* d) { return rows_workspace_floats(d, MODE_FWD); }, rows_prepare_batch,
     [](const ConvCall& c) { return run_rows(c, MODE_FWD); }, false},
    /* fwd_rd */ {fwd_rd_supported, NEED_NOTHING, packed, fwd_rd_prepared_floats, rd_prepare_batch,
     [](const ConvCall& c) {
         return fwd_rd_forward(c.d, c.in, c.prepared ? nullptr : c.w, c.prepared ? c.image() : nullptr, c.bias, c.out, c.out2, c.s);
     }, false},
    /* stem */ {stem_fwd_supported, NEED_NOTHING, copy_of_w, filter_floats, nullptr,
     [](const ConvCall& c) { return stem_forward(c.d, c.in, c.w_or_copy(), c.bias, c.out, c.out2, c.s); }, true},
    /* igemm */ {always, NEED_NOTHING,  // (the last route: a buffer that is too small is its error, not a fall-through)
     packed, [](const cnn_conv2d_desc* d) { return igemm_image_floats(d, MODE_FWD); }, igemm_prepare_batch,
     [](const ConvCall& c) { return igemm_run(c.who, c.d, MODE_FWD, c.in, c.w, c.bias, c.out, c.out2, c.ws, c.ws_bytes, c.s, c.prepared); }, false},
};

// ---- data gradient: depthwise (as above) -> direct -> 1x1 -> thin (packed, then scalar operands) -> rows -> dgrad_rd -> pk_s2 ->
// implicit GEMM ----
const Route kDgradRoutes[] = {
    /* depthwise */ {is_depthwise, NEED_NOTHING, no_image, no_floats, nullptr,
     [](const ConvCall& c) { return dw_run(c.d, MODE_DGRAD, c.in, c.w, nullptr, c.out, c.out2, c.s); }, false},
    /* direct */ {direct_conv_supported, NEED_NOTHING,
     [](const cnn_conv2d_desc* d) { return direct_dgrad_pk_ok(d) ? IMAGE_PACKED : IMAGE_NONE; }, direct_floats, direct_prepare_batch,
     [](const ConvCall& c) {  // the first-layer kernels have no masked epilogue: same result from the ReLU kernel
         const int rc = direct_conv_dgrad(c.d, c.in, c.w, c.out, c.ws, c.ws_bytes, c.s, c.prepared);
         if (rc || !c.out2) return rc;
         return cnn_relu_backward(c.out2, c.out, (size_t)c.d->B * c.d->Ci * c.d->H * c.d->W, c.s);
     }, false},
    /* 1x1 */ {c11_supported, NEED_NOTHING, copy_of_w, filter_floats, nullptr,
     [](const ConvCall& c) { return c11_backward_data(c.d, c.in, c.w_or_copy(), c.out2, c.out, c.s); }, false},
    /* thin_pk */ {[](const cnn_conv2d_desc* d) { return thin_dgrad_supported(d) && thin_dgrad_packed_floats(d) > 0; }, NEED_FLOATS, packed,
     thin_dgrad_packed_floats, thin_pack_jobs,
     [](const ConvCall& c) {
         if (!c.prepared)
             if (int rc = thin_dgrad_pack(c.d, c.w, (float*)c.ws, c.s)) return rc;
         return thin_dgrad(c.d, c.in, nullptr, c.image(), c.out2, c.out, c.s);
     }, false},
    /* thin */ {thin_dgrad_supported, NEED_NOTHING, copy_of_w, filter_floats, nullptr,
     [](const ConvCall& c) { return thin_dgrad(c.d, c.in, c.w_or_copy(), nullptr, c.out2, c.out, c.s); }, false},
    /* rows */ {[](const cnn_conv2d_desc* d) { return rows_workspace_floats(d, MODE_DGRAD) > 0; }, NEED_FLOATS_ALIGNED16, packed,
     [](const cnn_conv2d_desc* d) { return rows_workspace_floats(d, MODE_DGRAD); }, rows_prepare_batch,
     [](const ConvCall& c) { return run_rows(c, MODE_DGRAD); }, false},
    /* dgrad_rd */ {dgrad_rd_supported, NEED_NOTHING, packed, dgrad_rd_prepared_floats, rd_prepare_batch,
     [](const ConvCall& c) {
         return dgrad_rd_backward_data(c.d, c.in, c.prepared ? nullptr : c.w, c.prepared ? c.image() : nullptr, c.out2, c.out,
                                       c.prepared ? nullptr : c.ws, c.prepared ? 0 : c.ws_bytes, c.s);
     }, false},
    /* pk_s2 */ {pk_dgrad_s2_supported, NEED_FLOATS, packed, pk_dgrad_s2_workspace_floats, direct_prepare_batch,
     [](const ConvCall& c) { return pk_dgrad_s2(c.d, c.in, c.w, c.out, c.ws, c.s, c.prepared, c.out2); }, false},
    /* igemm */ {always, NEED_NOTHING, packed, [](const cnn_conv2d_desc* d) { return igemm_image_floats(d, MODE_DGRAD); }, igemm_prepare_batch,
     [](const ConvCall& c) { return igemm_run(c.who, c.d, MODE_DGRAD, c.in, c.w, c.bias, c.out, c.out2, c.ws, c.ws_bytes, c.s, c.prepared); }, false},
};

constexpr int kNumFwdRoutes = (int)(sizeof(kFwdRoutes) / sizeof(kFwdRoutes[0])), kNumDgradRoutes = (int)(sizeof(kDgradRoutes) / sizeof(kDgradRoutes[0]));
constexpr int kMaxRoutes = 9;
static_assert(kNumFwdRoutes <= kMaxRoutes && kNumDgradRoutes <= kMaxRoutes, "RouteFacts holds kMaxRoutes rows per pass");
const Route* routes(int mode) { return mode == MODE_FWD ? kFwdRoutes : kDgradRoutes; }
int num_routes(int mode) { return mode == MODE_FWD ? kNumFwdRoutes : kNumDgradRoutes; }

// What the tables say about one desc: asked once per (desc, option generation, tuner preference generation, CU count) and host
// thread, so that a launch costs one lookup here instead of every row's predicate and planner (the planning the size queries do
// once cost most of the host's enqueue time, see DescMemo).
struct RouteFacts {
    cnn_conv2d_desc d;
    unsigned gen, prefer_gen;
    int cus;
    bool used;
    struct {
        unsigned applies;  // bit i: row i covers the desc
        ImageKind image[kMaxRoutes];
        size_t floats[kMaxRoutes];
    } pass[2];
    size_t prepared_floats;  // the largest image of any row that applies, both passes
};
const RouteFacts& facts_of(const cnn_conv2d_desc* d) {
    static thread_local RouteFacts memo[16] = {};
    static thread_local int next = 0;
    const unsigned gen = options_generation(), prefer_gen = igemm_prefer_generation();
    const int cus = num_cus();
    for (const RouteFacts& f : memo)
        if (f.used && f.gen == gen && f.prefer_gen == prefer_gen && f.cus == cus && f.d.B == d->B && f.d.Ci == d->Ci && f.d.H == d->H &&
            f.d.W == d->W && f.d.Co == d->Co && f.d.k == d->k && f.d.s == d->s && f.d.pad == d->pad && f.d.flags == d->flags)
            return f;
    RouteFacts& f = memo[next];
    next = (next + 1) % 16;
    f = RouteFacts{*d, gen, prefer_gen, cus, true, {}, 0};
    for (int mode = 0; mode < 2; ++mode)
        for (int i = 0; i < num_routes(mode); ++i) {
            const Route& r = routes(mode)[i];
            if (!r.applies(d)) continue;
            f.pass[mode].applies |= 1u << i;
            f.pass[mode].image[i] = r.image(d);
            f.pass[mode].floats[i] = r.floats(d);
            if (f.pass[mode].floats[i] > f.prepared_floats) f.prepared_floats = f.pass[mode].floats[i];
            if (i == 0 && is_depthwise(d)) break;  // (the dense families' predicates and planners never see a depthwise desc)
        }
    return f;
}
size_t prepared_bytes_of(const RouteFacts& f) { return (f.prepared_floats + 64) * sizeof(float); }

// index of the first row of the pass that covers the desc and can live with the buffer; the last row of either table covers
// everything and asks for nothing (a buffer that is too small is its error, not a fall-through)
int resolve(int mode, const RouteFacts& f, const void* buf, size_t bytes) {
    const int last = num_routes(mode) - 1;
    for (int i = 0; i < last; ++i) {
        if (!(f.pass[mode].applies >> i & 1u)) continue;
        const BufferNeed need = routes(mode)[i].need;
        if (need == NEED_NOTHING) return i;
        if (buf != nullptr && bytes >= f.pass[mode].floats[i] * sizeof(float) && (need != NEED_FLOATS_ALIGNED16 || aligned16(buf))) return i;
    }
    return last;
}

// prepared: c.ws is a buffer of cnn_conv2d_prepared_bytes(d) bytes holding the route's image (c.ws_bytes is filled in here)
int run_pass(int mode, ConvCall c) {
    if (int rc = check_desc(c.who, c.d, c.prepared ? 0 : CNN_CONV2D_DEPTHWISE)) return rc;
    const RouteFacts& f = facts_of(c.d);
    if (c.prepared) c.ws_bytes = prepared_bytes_of(f);
    const int i = resolve(mode, f, c.ws, c.ws_bytes);
    const Route& r = routes(mode)[i];
    CNN_REQUIRE(!c.prepared || f.pass[mode].image[i] != IMAGE_NONE, "%s: no prepared path for this layer", c.who);
    // forward: y may be NULL when only the ReLU output is wanted and the route can write it alone
    CNN_REQUIRE(c.in && (c.w || c.prepared) && (mode == MODE_FWD ? (c.bias && (c.out || (c.out2 && !r.needs_y))) : c.out != nullptr),
                "%s: null pointer", c.who);
    return r.run(c);
}

}  // namespace

namespace cnn_amd {
// the largest image any route of either pass would keep in a prepared buffer (the caller sizes its buffers once, whatever the
// options and the tuner decide later: every implicit-GEMM tile candidate is counted)
size_t igemm_workspace_floats(const cnn_conv2d_desc* d) { return facts_of(d).prepared_floats; }
}  // namespace cnn_amd

extern "C" {

int cnn_conv2d_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y,
                       void* ws, size_t ws_bytes, void* stream) {
    return run_pass(MODE_FWD, ConvCall{"cnn_conv2d_forward", d, x, w, bias, y, nullptr, ws, ws_bytes, as_stream(stream), false});
}

int cnn_conv2d_forward_relu(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y,
                            float* y_relu, void* ws, size_t ws_bytes, void* stream) {
    CNN_REQUIRE(y_relu, "cnn_conv2d_forward_relu: null pointer");
    return run_pass(MODE_FWD, ConvCall{"cnn_conv2d_forward_relu", d, x, w, bias, y, y_relu, ws, ws_bytes, as_stream(stream), false});
}

int cnn_conv2d_forward_prepared(const cnn_conv2d_desc* d, const float* x, const void* prepared_fwd, const float* bias, float* y,
                                float* y_relu, void* stream) {
    CNN_REQUIRE(prepared_fwd != nullptr, "cnn_conv2d_forward_prepared: null pointer");
    return run_pass(MODE_FWD, ConvCall{"cnn_conv2d_forward_prepared", d, x, nullptr, bias, y, y_relu, (void*)prepared_fwd, 0, as_stream(stream), true});
}

// relu_below (nullable): output of the ReLU layer whose input gradient dx is -- fuses that layer's backward pass
int cnn_conv2d_backward_data(const cnn_conv2d_desc* d, const float* dy, const float* w, float* dx, void* ws,
                             size_t ws_bytes, void* stream) {
    return run_pass(MODE_DGRAD, ConvCall{"cnn_conv2d_backward_data", d, dy, w, nullptr, dx, nullptr, ws, ws_bytes, as_stream(stream), false});
}

int cnn_conv2d_backward_data_relu(const cnn_conv2d_desc* d, const float* dy, const float* w, const float* relu_below, float* dx,
                                  void* ws, size_t ws_bytes, void* stream) {
    CNN_REQUIRE(relu_below, "cnn_conv2d_backward_data_relu: null pointer");
    return run_pass(MODE_DGRAD, ConvCall{"cnn_conv2d_backward_data_relu", d, dy, w, nullptr, dx, const_cast<float*>(relu_below), ws, ws_bytes,
                                         as_stream(stream), false});
}

int cnn_conv2d_backward_data_relu_prepared(const cnn_conv2d_desc* d, const float* dy, const void* prepared_dgrad,
                                           const float* relu_below, float* dx, void* stream) {
    CNN_REQUIRE(prepared_dgrad != nullptr && relu_below != nullptr, "cnn_conv2d_backward_data_relu_prepared: null pointer");
    return run_pass(MODE_DGRAD, ConvCall{"cnn_conv2d_backward_data_relu_prepared", d, dy, nullptr, nullptr, dx, const_cast<float*>(relu_below),
                                         (void*)prepared_dgrad, 0, as_stream(stream), true});
}

int cnn_conv2d_backward_data_prepared(const cnn_conv2d_desc* d, const float* dy, const void* prepared_dgrad, float* dx,
                                      void* stream) {
    CNN_REQUIRE(prepared_dgrad != nullptr, "cnn_conv2d_backward_data_prepared: null pointer");
    return run_pass(MODE_DGRAD, ConvCall{"cnn_conv2d_backward_data_prepared", d, dy, nullptr, nullptr, dx, nullptr, (void*)prepared_dgrad, 0,
                                         as_stream(stream), true});
}

int cnn_conv2d_relu_only_supported(const cnn_conv2d_desc* d) {
    if (check_desc("cnn_conv2d_relu_only_supported", d)) return 0;
    // (every family behind cnn_conv2d_forward except the thin first layers'; asked of the route a buffer of any size resolves to)
    alignas(16) static const char any_buffer[16] = {};
    return kFwdRoutes[resolve(MODE_FWD, facts_of(d), any_buffer, ~(size_t)0 / 2)].needs_y ? 0 : 1;
}

/* ---- Conv2D -> ReLU -> MaxPool2D(2,2) ---- */
int cnn_conv2d_relu_maxpool2_supported(const cnn_conv2d_desc* d) {
    if (check_desc("cnn_conv2d_relu_maxpool2_supported", d)) return 0;
    return direct_conv_pool_supported(d) ? 1 : 0;
}

int cnn_conv2d_pool_mask_packed_supported(const cnn_conv2d_desc* d) {
    if (check_desc("cnn_conv2d_pool_mask_packed_supported", d)) return 0;
    return direct_pool_mask_packed_ok(d) ? 1 : 0;
}
size_t cnn_conv2d_pool_mask_bytes(const cnn_conv2d_desc* d) {
    if (check_desc("cnn_conv2d_pool_mask_bytes", d)) return 0;
    return direct_pool_mask_bytes(d);
}
int cnn_conv2d_pool_mask_unpack(const cnn_conv2d_desc* d, const void* packed, int32_t* mask, void* stream) {
    if (int rc = check_desc("cnn_conv2d_pool_mask_unpack", d)) return rc;
    CNN_REQUIRE(packed && mask, "cnn_conv2d_pool_mask_unpack: null pointer");
    return direct_pool_mask_unpack(d, packed, mask, as_stream(stream));
}

int cnn_conv2d_relu_maxpool2_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* pooled,
                                     int32_t* mask, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_desc("cnn_conv2d_relu_maxpool2_forward", d)) return rc;
    CNN_REQUIRE(x && w && bias && pooled, "cnn_conv2d_relu_maxpool2_forward: null pointer");
    return direct_conv_pool_forward(d, x, w, bias, pooled, mask, ws, ws_bytes, as_stream(stream), false);
}

int cnn_conv2d_relu_maxpool2_forward_prepared(const cnn_conv2d_desc* d, const float* x, const void* prepared_fwd, float* pooled,
                                              int32_t* mask, void* stream) {
    if (int rc = check_desc("cnn_conv2d_relu_maxpool2_forward_prepared", d)) return rc;
    CNN_REQUIRE(x && prepared_fwd && pooled, "cnn_conv2d_relu_maxpool2_forward_prepared: null pointer");
    return direct_conv_pool_forward(d, x, nullptr, nullptr, pooled, mask, (void*)prepared_fwd, cnn_conv2d_prepared_bytes(d),
                                    as_stream(stream), true);
}

int cnn_conv2d_backward_data_pooled2(const cnn_conv2d_desc* d, const float* dpool, const int32_t* mask, const float* pooled,
                                     const float* w, float* dx, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_desc("cnn_conv2d_backward_data_pooled2", d)) return rc;
    CNN_REQUIRE(dpool && mask && w && dx, "cnn_conv2d_backward_data_pooled2: null pointer");
    return direct_conv_dgrad_pooled(d, dpool, mask, pooled, w, dx, ws, ws_bytes, as_stream(stream), false);
}

int cnn_conv2d_backward_data_pooled2_prepared(const cnn_conv2d_desc* d, const float* dpool, const int32_t* mask, const float* pooled,
                                              const void* prepared_dgrad, float* dx, void* stream) {
    if (int rc = check_desc("cnn_conv2d_backward_data_pooled2_prepared", d)) return rc;
    CNN_REQUIRE(dpool && mask && prepared_dgrad && dx, "cnn_conv2d_backward_data_pooled2_prepared: null pointer");
    return direct_conv_dgrad_pooled(d, dpool, mask, pooled, nullptr, dx, (void*)prepared_dgrad, cnn_conv2d_prepared_bytes(d),
                                    as_stream(stream), true);
}

/* ---- filter preparation hoisted out of the per-layer calls ---- */
size_t cnn_conv2d_prepared_bytes(const cnn_conv2d_desc* d) {
    if (check_desc("cnn_conv2d_prepared_bytes", d)) return 0;
    return prepared_bytes_of(facts_of(d));
}

// Every (layer, pass) with a buffer is one job.  It resolves exactly as the *_prepared call on that buffer will (same pointer, same
// cnn_conv2d_prepared_bytes), a verbatim-copy image is copied here, and each batch preparer gets the jobs of its routes in one call.
int cnn_conv2d_prepare_filters(int n, const cnn_conv2d_desc* descs, const float* const* w, const float* const* bias,
                               void* const* fwd, void* const* dgrad, void* stream) {
    CNN_REQUIRE(n > 0 && n <= kMaxPrepLayers && descs && w && bias, "cnn_conv2d_prepare_filters: n=%d (1..6 layers per call)", n);
    hipStream_t s = as_stream(stream);
    ConvPrepJob jobs[kMaxPrepJobs];
    PrepareBatchFn prepare[kMaxPrepJobs];
    int nj = 0;
    for (int i = 0; i < n; ++i) {
        const cnn_conv2d_desc* d = &descs[i];
        if (int rc = check_desc("cnn_conv2d_prepare_filters", d)) return rc;
        const RouteFacts& f = facts_of(d);
        for (int mode = 0; mode < 2; ++mode) {
            void* out = mode == MODE_FWD ? (fwd ? fwd[i] : nullptr) : (dgrad ? dgrad[i] : nullptr);
            if (!out) continue;
            CNN_REQUIRE(w[i] != nullptr, "cnn_conv2d_prepare_filters: filters of layer %d are null", i);
            const int ri = resolve(mode, f, out, prepared_bytes_of(f));
            const ImageKind kind = f.pass[mode].image[ri];
            CNN_REQUIRE(kind != IMAGE_NONE, "cnn_conv2d_prepare_filters: layer %d has no prepared path for this mode", i);
            if (kind == IMAGE_COPY_OF_W) {
                CNN_HIP_CHECK(hipMemcpyAsync(out, w[i], sizeof(float) * f.pass[mode].floats[ri], hipMemcpyDeviceToDevice, s));
                continue;
            }
            prepare[nj] = routes(mode)[ri].prepare;
            jobs[nj++] = ConvPrepJob{d, i, mode, w[i], bias[i], (float*)out};
        }
    }
    for (int i = 0; i < nj; ++i) {
        if (!prepare[i]) continue;  // (went with an earlier job's batch)
        const PrepareBatchFn fn = prepare[i];
        ConvPrepJob batch[kMaxPrepJobs];
        int nb = 0;
        for (int k = i; k < nj; ++k)
            if (prepare[k] == fn) {
                batch[nb++] = jobs[k];
                prepare[k] = nullptr;
            }
        if (int rc = fn(nb, batch, s)) return rc;
    }
    return CNN_AMD_OK;
}

}  // extern "C"
