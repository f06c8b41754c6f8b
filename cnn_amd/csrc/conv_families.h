// conv_families.h -- what the Conv2D translation units know of each other: every function one conv_*.hip file calls in
// another is declared HERE and nowhere else (a changed signature is a compile error in both files, not a link error or a
// silent mismatch), with the geometry tag of the kernel-timing log and the descriptor check of the C entry points.
// Who calls whom: conv_dispatch.hip (forward / data-gradient routes) and conv_wgrad.hip (weight-gradient slab
// families) call the families; the families call back only for igemm_preferred and for their own siblings.
#pragma once
#include "common.h"

// printf-style geometry tag of a launch (CNN_KLAUNCH's trailing arguments); format and arguments apart for a family that appends to it
#define CONV_TAG_FMT "B%d Ci%d %dx%d Co%d k%d s%d p%d"
#define CONV_TAG_ARGS(d) (d)->B, (d)->Ci, (d)->H, (d)->W, (d)->Co, (d)->k, (d)->s, (d)->pad
#define CONV_TAG(d) CONV_TAG_FMT, CONV_TAG_ARGS(d)

namespace cnn_amd {

enum { MODE_FWD = 0, MODE_DGRAD = 1 };  // the `mode` argument below: forward / data gradient

// every C entry point that takes a desc starts with this.  accepted_extra: the flag bits beyond the pool-mask one that the entry
// serves (CNN_CONV2D_DEPTHWISE for the entries listed in include/cnn_amd.h, 0 everywhere else: those refuse a depthwise desc here,
// before any launch)
inline int check_desc(const char* who, const cnn_conv2d_desc* d, int accepted_extra = 0) {
    CNN_REQUIRE(d != nullptr, "%s: desc is null", who);
    CNN_REQUIRE(d->B > 0 && d->Ci > 0 && d->H > 0 && d->W > 0 && d->Co > 0 && d->k > 0 && d->s > 0 && d->pad >= 0,
                "%s: bad desc B=%d Ci=%d H=%d W=%d Co=%d k=%d s=%d pad=%d", who, d->B, d->Ci, d->H, d->W, d->Co, d->k,
                d->s, d->pad);
    CNN_REQUIRE(d->H + 2 * d->pad >= d->k && d->W + 2 * d->pad >= d->k, "%s: kernel %d larger than padded input", who,
                d->k);
    CNN_REQUIRE((d->flags & ~(CNN_CONV2D_POOL_MASK_PACKED | CNN_CONV2D_DEPTHWISE)) == 0, "%s: unknown desc flags 0x%x", who, (unsigned)d->flags);
    if (d->flags & CNN_CONV2D_DEPTHWISE) {
        CNN_REQUIRE((accepted_extra & CNN_CONV2D_DEPTHWISE) != 0, "%s: no depthwise path (CNN_CONV2D_DEPTHWISE is served by the plain forward / backward entries only)", who);
        CNN_REQUIRE(d->flags == CNN_CONV2D_DEPTHWISE, "%s: depthwise desc with other flags 0x%x", who, (unsigned)d->flags);
        CNN_REQUIRE(d->Co == d->Ci, "%s: depthwise needs Co == Ci (Ci=%d Co=%d)", who, d->Ci, d->Co);
        // the depthwise kernels index in 32 bits
        const double Ho = cnn_conv2d_out_dim(d->H, d->k, d->s, d->pad), Wo = cnn_conv2d_out_dim(d->W, d->k, d->s, d->pad);
        const double planes = (double)d->B * d->Ci;  // (doubles: the products of four ints overflow 64 bits)
        CNN_REQUIRE(planes * d->H * d->W < 2147483648.0 && planes * Ho * Wo < 2147483648.0,
                    "%s: depthwise tensors must have fewer than 2^31 elements (B=%d C=%d %dx%d)", who, d->B, d->Ci, d->H, d->W);
    }
    return CNN_AMD_OK;
}
inline bool is_depthwise(const cnn_conv2d_desc* d) { return (d->flags & CNN_CONV2D_DEPTHWISE) != 0; }

// one filter-preparation job of cnn_conv2d_prepare_filters: layer `layer` of the call, its image for `mode` goes to `image`.
// A family's batch preparer gets the jobs that resolved to it (conv_dispatch.hip) and serves them in one launch.
struct ConvPrepJob {
    const cnn_conv2d_desc* d;
    int layer, mode;
    const float* w;
    const float* bias;
    float* image;
};
constexpr int kMaxPrepLayers = 6;                   // layers per cnn_conv2d_prepare_filters call
constexpr int kMaxPrepJobs = 2 * kMaxPrepLayers;    // one job per layer and mode

// ---- conv_igemm.hip: the implicit GEMM (every geometry; the last route of both passes) and its tuner ----
// floats of the largest filter image (+ split-K partial tensors) any tile the tuner may pin needs in `mode`
size_t igemm_image_floats(const cnn_conv2d_desc* d, int mode);
// forward: in = x, out = y, out2 = relu(y) (nullable); data gradient: in = dy, out = dx, out2 = the ReLU output below (nullable).
// prepared: `ws` already holds the filter image, w is unused
int igemm_run(const char* who, const cnn_conv2d_desc* d, int mode, const float* in, const float* w, const float* bias, float* out,
              float* out2, void* ws, size_t ws_bytes, hipStream_t s, bool prepared);
int igemm_prepare_batch(int n, const ConvPrepJob* jobs, hipStream_t s);
bool igemm_preferred(const cnn_conv2d_desc* d, int mode);  // the tuner measured the implicit GEMM faster than the register-direct kernel
unsigned igemm_prefer_generation();                        // moves whenever an igemm_preferred answer may have changed

// ---- conv_dispatch.hip ----
size_t igemm_workspace_floats(const cnn_conv2d_desc* d);  // the largest prepared image of any route of either pass

// ---- conv_direct.hip: the thin first layer (3 -> 16, 3x3, stride 2, pad 0) and the packed stride-2 data gradient ----
bool direct_conv_supported(const cnn_conv2d_desc* d);
bool direct_fwd_pk_ok(const cnn_conv2d_desc* d);    // the packed forward kernel applies: the only one that reads a prepared image
bool direct_dgrad_pk_ok(const cnn_conv2d_desc* d);  // the same for the data gradient
int direct_conv_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y, float* y_relu,
                        void* ws, size_t ws_bytes, hipStream_t s, bool prepared);
int direct_conv_dgrad(const cnn_conv2d_desc* d, const float* dy, const float* w, float* dx, void* ws, size_t ws_bytes,
                      hipStream_t s, bool prepared);
int direct_prepare_batch(int n, const ConvPrepJob* jobs, hipStream_t s);  // direct forward / data gradient and pk_s2 jobs
bool direct_conv_pool_supported(const cnn_conv2d_desc* d);  // Conv -> ReLU -> MaxPool(2,2) in one kernel
bool direct_pool_mask_packed_ok(const cnn_conv2d_desc* d);
size_t direct_pool_mask_bytes(const cnn_conv2d_desc* d);
int direct_pool_mask_unpack(const cnn_conv2d_desc* d, const void* packed, int32_t* mask, hipStream_t s);
int direct_conv_pool_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* pooled,
                             int32_t* mask, void* ws, size_t ws_bytes, hipStream_t s, bool prepared);
int direct_conv_dgrad_pooled(const cnn_conv2d_desc* d, const float* dpool, const int32_t* mask, const float* pooled, const float* w,
                             float* dx, void* ws, size_t ws_bytes, hipStream_t s, bool prepared);
bool pk_dgrad_s2_supported(const cnn_conv2d_desc* d);  // packed VALU data gradient of small 3x3 / stride-2 layers
size_t pk_dgrad_s2_workspace_floats(const cnn_conv2d_desc* d);
int pk_dgrad_s2(const cnn_conv2d_desc* d, const float* dy, const float* w, float* dx, void* ws, hipStream_t s, bool prepared,
                const float* relu_below);
int direct_wgrad_slots(const cnn_conv2d_desc* d);  // slabs of [16][27 | 1] floats
int direct_conv_wgrad(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);
int direct_conv_wgrad_pooled(const cnn_conv2d_desc* d, const float* x, const float* dpool, const int32_t* mask, const float* pooled,
                             float* slabs, hipStream_t s);
int direct_first_layer_finish(const cnn_conv2d_desc* d, const float* slabs, int nslots, float divisor, float* gw, float* gb, float* w,
                              float* bias, float lr, float grad_scale, void* fwd_img, void* dgrad_img, float* w_keep, float* bias_keep,
                              hipStream_t s);

// ---- conv_wgrad_win.hip: the window-major MFMA weight gradient of the first layer (behind direct_conv_wgrad*) ----
int win_wgrad_slots(const cnn_conv2d_desc* d);
int win_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, const int32_t* mask, const float* pooled, float* slabs,
                     hipStream_t s);

// ---- conv_1x1.hip: 1x1 convolutions (stride 1 / 2) as LDS-tiled GEMMs; they read the reference filter layout ----
bool c11_supported(const cnn_conv2d_desc* d);
int c11_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y, float* y_relu, hipStream_t s);
int c11_backward_data(const cnn_conv2d_desc* d, const float* dy, const float* w, const float* relu_below, float* dx, hipStream_t s);
int c11_wgrad_slots(const cnn_conv2d_desc* d);  // slabs of [Co][Ci | 1]
int c11_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);

// ---- conv_rows.hip (with conv_rows_s2.hip, conv_rows_any.hip behind it): LDS-staged 3x3 forward and data gradient ----
size_t rows_workspace_floats(const cnn_conv2d_desc* d, int mode);  // floats of the filter image, 0: not covered in that mode
int rows_prepare(const cnn_conv2d_desc* d, int mode, const float* w, float* image, hipStream_t s);
int rows_prepare_batch(int n, const ConvPrepJob* jobs, hipStream_t s);
int rows_run(const cnn_conv2d_desc* d, int mode, const float* in, const float* image, const float* bias, float* out, float* out_relu,
             const float* relu_below, hipStream_t s);
bool s2_info(const cnn_conv2d_desc* d, int mode, int* mt, int* qw, int* ck, int* nchunk, int* ntiles, size_t* wt_floats);
int s2_run(const cnn_conv2d_desc* d, int mode, const float* in, const float* image, const float* bias, float* out, float* out_relu,
           const float* relu_below, hipStream_t s);
bool any_info(const cnn_conv2d_desc* d, int mode, int* mt, int* qw, int* ck, int* nchunk, int* ntiles, size_t* wt_floats);
int any_run(const cnn_conv2d_desc* d, int mode, const float* in, const float* image, const float* bias, float* out, float* out_relu,
            const float* relu_below, hipStream_t s);

// ---- conv_fwd_rd.hip: register-direct forward of the 3x3 / pad-0 layers with 16 / 32 / 64 input channels ----
bool fwd_rd_supported(const cnn_conv2d_desc* d);
bool fwd_rd_small(const cnn_conv2d_desc* d);  // the small-layer kernel (never replaced by the implicit GEMM)
size_t fwd_rd_prepared_floats(const cnn_conv2d_desc* d);
int fwd_rd_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* img, const float* bias, float* y,
                   float* y_relu, hipStream_t s);
int rd_prepare_batch(int n, const ConvPrepJob* jobs, hipStream_t s);  // fwd_rd forward images and dgrad_rd filter copies

// ---- conv_dgrad_rd.hip: register-direct data gradient (3x3, stride 1 / 2, Co 32 / 64 / 128) ----
bool dgrad_rd_supported(const cnn_conv2d_desc* d);
size_t dgrad_rd_prepared_floats(const cnn_conv2d_desc* d);
int dgrad_rd_prepare_layout(const cnn_conv2d_desc* d, int* transposed);  // 0: not covered
int dgrad_rd_backward_data(const cnn_conv2d_desc* d, const float* dy, const float* w, const float* img, const float* relu_below,
                           float* dx, void* ws, size_t ws_bytes, hipStream_t s);

// ---- conv_stem.hip: 3 -> Co, 7x7, stride 2, pad 3; reads the reference filter layout ----
bool stem_fwd_supported(const cnn_conv2d_desc* d);
int stem_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y, float* y_relu, hipStream_t s);
int stem_wgrad_slots(const cnn_conv2d_desc* d);  // slabs of [Co][147 | 1]
int stem_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);

// ---- conv_dgrad_thin.hip: VALU data gradient of the thin (Ci = 3) layers ----
bool thin_dgrad_supported(const cnn_conv2d_desc* d);
size_t thin_dgrad_packed_floats(const cnn_conv2d_desc* d);  // > 0: the layer has a packed filter image (the 7x7 stem) ...
int thin_dgrad_pack(const cnn_conv2d_desc* d, const float* w, float* image, hipStream_t s);  // ... made by this
int thin_dgrad(const cnn_conv2d_desc* d, const float* dy, const float* w, const float* packed, const float* relu_below, float* dx,
               hipStream_t s);

// ---- weight-gradient slab families: *_slots = partial slabs the kernel writes (0: not covered), *_launch writes them ----
int os_wgrad_slots(const cnn_conv2d_desc* d);  // conv_wgrad_os.hip: small 3x3 / stride-2 layers, output-stationary; [Co][Ci*9 | 1]
int os_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);
int sp_wgrad_slots(const cnn_conv2d_desc* d);  // conv_wgrad_sp.hip: small planes, 3x3, LDS-staged output-stationary; [Co][Ci*9 | 1]
int sp_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);
int sp2_wgrad_slots(const cnn_conv2d_desc* d);  // conv_wgrad_sp2.hip: its stride-2 sibling, behind sp_wgrad_*
int sp2_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);
int spa_wgrad_slots(const cnn_conv2d_desc* d);  // conv_wgrad_sp_any.hip: its runtime-size sibling, behind sp_wgrad_*
int spa_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);
int wgrad_rd_slots(const cnn_conv2d_desc* d);  // conv_wgrad_rd.hip: register-direct MFMA kernel (3x3, pad 0); [Co][Ci*9 | 1]
int wgrad_rd_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);
int wgrad_rd_pooled_slots(const cnn_conv2d_desc* d);
int wgrad_rd_launch_pooled(const cnn_conv2d_desc* d, const float* x, const float* dpool, const int32_t* mask, const float* pooled,
                           float* slabs, hipStream_t s);

// ---- conv_depthwise.hip: CNN_CONV2D_DEPTHWISE, every pass (VALU, HBM-bound).  w is [C][1][k][k] ----
// forward: out = y (nullable when out2 is given), out2 = relu(y) (nullable); data gradient: out = dx, out2 = the ReLU output below (nullable)
int dw_run(const cnn_conv2d_desc* d, int mode, const float* in, const float* w, const float* bias, float* out, float* out2, hipStream_t s);
int dw_wgrad_slots(const cnn_conv2d_desc* d);  // batch slabs of [C][k*k | 1] floats (planned by num_cus())
int dw_wgrad_launch(const cnn_conv2d_desc* d, const float* x, const float* dy, float* slabs, hipStream_t s);

// ---- conv_wgrad.hip, for conv_backward.hip: record (true) / launch at once (false) the final slab reductions of this thread ----
void wgrad_defer_reduce(bool on);
int wgrad_flush_reduces(hipStream_t s);

}  // namespace cnn_amd
